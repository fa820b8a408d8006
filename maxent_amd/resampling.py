"""Jackknife and bootstrap error bars from Monte Carlo bins (``TauMaxEnt.resample_errors``,
``ElementwiseMaxEnt.resample_errors``).  Not in the reference, whose users loop ``run()`` over their resamples.

Every resample of the bins is continued like the full sample and the spread of whatever is wanted is taken: A(omega),
spectral weights, functionals, the alpha the analyzer picks -- and, with ``keep_samples``, anything nonlinear
downstream.  Where :mod:`maxent_amd.posterior` expands around one minimiser at a fixed alpha, this needs no
expansion, covers the uncertainty of the alpha selection (``alpha_mode='per_resample'``) and costs n_res scans.

All resamples of a matrix element share its covariance -- the one of the full sample, as ``set_G_*_bins`` staged it
-- and so ONE data set on the device; only the rotated data differ.  They come from ``mxe_bins_resample`` (all sets
of the job in one launch), the n_res x n_elem scans are one launch of the solver per device, the device picks every
scan's alpha (``mxe_select3_launch``), and ``mxe_resample_reduce`` reads the chosen H rows where they lie: no H row
of a resample crosses to the host unless ``keep_samples`` asks for them.  This module is the host glue: the tables
of multiplicities, which rows form which group, the shape of what is returned.  There is no CPU path.
"""

import numpy as np

from . import device
from .posterior import window_rows, functional_rows, rows_on_H

#: the analyzers whose alpha the device picks behind the solve, in the order of ``mxe_select3_launch``
SLOTS = ('LineFitAnalyzer', 'Chi2CurvatureAnalyzer', 'EntropyAnalyzer')
#: rows of a preblur matrix that go through ``mxe_resample_reduce`` at a time (their covariance block is formed and dropped)
BLUR_CHUNK = 32


# ---- tables of multiplicities (no device) -----------------------------------------------------------------------------

def jackknife_counts(n_bins, block=1):
    """leave-one-block-out: ``n_bins // block`` rows of n_bins multiplicities, row r with the bins
    ``r block .. (r + 1) block - 1`` at 0 and every other at 1; trailing bins beyond the last whole block stay in every
    resample.  Fewer than two resamples raise."""
    n_bins, block = int(n_bins), int(block)
    if block < 1:
        raise ValueError('jackknife: block = {} (at least 1 is needed)'.format(block))
    n_res = n_bins // block
    if n_res < 2:
        raise ValueError('jackknife: {} bins in blocks of {} give {} resample(s); at least two are needed'.format(
            n_bins, block, n_res))
    counts = np.ones((n_res, n_bins), dtype=np.int32)
    for r in range(n_res):
        counts[r, r * block:(r + 1) * block] = 0
    return counts


def bootstrap_counts(n_bins, n_resamples, seed):
    """``n_resamples`` draws of n_bins bins with replacement:
    ``numpy.random.default_rng(seed).multinomial(n_bins, ones / n_bins, size=n_resamples)``; ``seed`` is required"""
    if seed is None:
        raise ValueError('bootstrap: a seed is required (the resamples must be reproducible)')
    n_bins = int(n_bins)
    if n_resamples is None or int(n_resamples) < 2:
        raise ValueError('bootstrap: n_resamples = {} (at least two are needed)'.format(n_resamples))
    if n_bins < 2:
        raise ValueError('bootstrap: {} bin(s); at least two are needed'.format(n_bins))
    rng = np.random.default_rng(seed)
    return rng.multinomial(n_bins, np.ones(n_bins) / n_bins, size=int(n_resamples)).astype(np.int32)


def resample_counts(method, n_bins, block=1, n_resamples=None, seed=None):
    """the table ``mxe_bins_resample`` takes: a leading row of ones -- the full sample, chain 0 of every element --,
    then the rows of :func:`jackknife_counts` or :func:`bootstrap_counts`"""
    if method == 'jackknife':
        rows = jackknife_counts(n_bins, block)
    elif method == 'bootstrap':
        rows = bootstrap_counts(n_bins, n_resamples, seed)
    else:
        raise ValueError("method={!r}: 'jackknife' or 'bootstrap'".format(method))
    return np.concatenate([np.ones((1, int(n_bins)), dtype=np.int32), rows])


def spread_scale(method, n_used):
    """the factor on the centred sum of squares of ``n_used`` resamples: (n - 1) / n jackknife, 1 / (n - 1) bootstrap and
    parametric bootstrap (1 where fewer than two are left: the variances are NaN then)"""
    n = float(n_used)
    if n < 2:
        return 1.0
    return (n - 1.0) / n if method == 'jackknife' else 1.0 / (n - 1.0)


def choose_slot(alpha, analyzers, n_alpha):
    """``alpha=`` of resample_errors -> (slot of ``SLOTS`` or None, fixed index or None)"""
    if alpha is None:
        name = analyzers[0].name if analyzers else None
        if name not in SLOTS:
            raise ValueError('the default analyzer {!r} is not one of {}: give alpha= one of them or an index'.format(
                name, ', '.join(SLOTS)))
        return SLOTS.index(name), None
    if isinstance(alpha, str):
        name = alpha if alpha.endswith('Analyzer') else alpha + 'Analyzer'
        if name not in SLOTS:
            raise ValueError('alpha={!r}: one of {} or an index is needed'.format(alpha, ', '.join(SLOTS)))
        return SLOTS.index(name), None
    if np.ndim(alpha) != 0:
        raise ValueError('alpha={!r}: an analyzer name or ONE index is needed'.format(alpha))
    i = int(alpha)
    if not -n_alpha <= i < n_alpha:
        raise ValueError('alpha index {} out of range for {} alphas'.format(i, n_alpha))
    return None, i % n_alpha


def check_minimizer(loop):
    if not hasattr(loop.minimizer, 'to_opts'):
        raise NotImplementedError('resample_errors needs the device solver: a user-supplied Minimizer works on one cost '
                                  'function at a time and cannot take the resamples as one launch')


def padded_T(st, n_data):
    """the eigenvector rows of ``bin_statistics`` as ``mxe_bins_eig`` wrote them: zero rows behind the kept ones"""
    T = np.zeros((n_data, n_data))
    T[:st['rank']] = st['T']
    return T


# ---- the device part: the scans of all resamples of several elements of one kernel -------------------------------------

def element_resamples(K, omega, loop, templates, G_rows, method, alpha=None, alpha_mode='per_resample', windows=None,
                      functionals=None, pointwise=True, keep_samples=False, device_ids=None, quantiles=None):
    """The resampling errors of the elements ``templates`` (their specs, as ``MaxEntLoop.make_spec`` makes them) of one
    kernel.  ``G_rows[e]``: (1 + n_res, rank_e) rotated data of element e, row 0 the full sample.  Element e is solved on
    device e mod N -- all its chains on that device, one launch per device -- and reduced there.  Returns (list of dicts,
    one per element, info).

    ``method``: ``'jackknife'``, ``'bootstrap'`` or ``'parametric'`` (rows 1 .. are mock data, :mod:`maxent_amd.mock`: the
    spread scale of the bootstrap, no jackknife bias, and the chi2 of every scan at its pick as ``chi2_scans``).
    ``quantiles``: probabilities in [0, 1] -> ``quantiles``, ``A_quantiles`` (n_q, n_omega; with ``pointwise``),
    ``window_quantiles``, ``functional_quantiles`` (n_q, n): type-7 quantiles (numpy's default) over the resamples that
    were used.  The bands of the hidden image come from ``mxe_resample_quantiles`` on the same groups, read where the rows
    lie.  With a ``PreblurKernel`` the bands must refer to A = B H, which is no row of the launch: they go the ``BLUR_CHUNK``
    way of the means -- the values of a chunk of rows of B on every resample from ``mxe_resample_reduce``, the quantile of
    those few numbers taken on the host; the device kernel serves the plain case.  The quantiles of windows and
    functionals are taken on the host from the values that are returned anyway."""
    from .batch_solver import BatchSolver, directions_to_keep
    from .maxent_loop import solve_elements, select_params
    if alpha_mode not in ('per_resample', 'full_sample'):
        raise ValueError("alpha_mode={!r}: 'per_resample' or 'full_sample'".format(alpha_mode))
    check_minimizer(loop)
    delta = np.asarray(omega.delta, dtype=float)
    n_omega = len(delta)
    n_elem, n_tot = len(templates), int(G_rows[0].shape[0])
    n_res = n_tot - 1
    quantiles = check_quantiles(quantiles, method, n_res)
    n_alpha = len(templates[0]['alpha'])
    n_win = 0 if windows is None else len(windows)
    Wrows = window_rows(omega, windows) if n_win else np.zeros((0, n_omega))
    Frows = functional_rows(functionals, n_omega) if functionals is not None else np.zeros((0, n_omega))
    n_fun = len(Frows)
    if n_win + n_fun == 0 and not pointwise and not keep_samples:
        raise ValueError('nothing to compute: give windows=, functionals=, pointwise=True or keep_samples=True')
    B = loop.A_of_H.matrix()
    rows = rows_on_H(np.concatenate([Wrows, Frows]), delta, B)          # weights on H (with a preblur: on A = B H)
    n_f = len(rows)
    slot, fixed = choose_slot(alpha, loop.analyzers, n_alpha)
    sel = select_params(loop.analyzers)
    deg, gamma = (sel[0], sel[1]) if sel is not None else (0, 0.2)
    # (the fourth entry: the rows of the picks stay on the device -- mxe_resample_reduce reads them there)
    select = (deg, gamma, slot if slot is not None else 0, False)
    ids = tuple(device_ids) if device_ids else (loop.device_id,)
    N = len(ids)
    per_dev = [[e for e in range(n_elem) if e % N == r] for r in range(N)]
    outs = [None] * n_elem
    info = dict(kernel_ms=0.0, reduce_ms=0.0, launches=0, reduce_launches=0, n_datasets=0, devices=[], left_out={})
    begun = []
    try:
        for r, dev in enumerate(ids):
            if not per_dev[r]:
                continue
            specs = [loop.spec_like(templates[e], G_rows[e][k], templates[e]['err']) for e in per_dev[r] for k in range(n_tot)]
            solver = BatchSolver.for_kernel(K, (dev,), keep=directions_to_keep(K, specs, None, chi2_factor=loop.cost_function.chi2_factor))
            solver._lock.acquire()              # (until this device's rows are reduced: nobody else launches on its contexts)
            begun.append([r, solver, specs, None])
            begun[-1][3] = solve_elements(K, specs, loop.minimizer, device_ids=(dev,),
                                          chi2_factor=loop.cost_function.chi2_factor, select=select, want_H=False, defer=True)
        for entry in begun:
            r, solver, specs, end = entry
            entry[3] = None
            sols, launch = end()
            if solver.last_info is not launch:
                # (solve_elements asks the pool for the solver of (K, device) itself: it must have been handed the one that is
                #  locked here, or the rows reduced below would be those of another launch)
                raise RuntimeError('resample_errors: the launch ran on another solver than the one that was locked')
            info['kernel_ms'] = max(info['kernel_ms'], launch.get('kernel_ms', 0.0))
            info['launches'] += 1
            info['n_datasets'] += int(np.sum(launch.get('n_datasets', 0)))
            info['devices'].append(ids[r])
            for k in ('audit_max', 'audit_problems'):
                if k in launch:
                    info[k] = max(info.get(k, 0.0), launch[k]) if k == 'audit_max' else info.get(k, 0) + launch[k]
            mine = per_dev[r]
            if fixed is None:
                picks = np.array([int(s['device_select']['index'][slot]) for s in sols], dtype=np.int64).reshape(len(mine), n_tot)
            else:
                picks = np.full((len(mine), n_tot), fixed, dtype=np.int64)
            if alpha_mode == 'full_sample':
                picks = np.repeat(picks[:, :1], n_tot, axis=1)
            got = _reduce_device(solver.ctxs[0], picks, n_alpha, method, rows, B if pointwise else None, pointwise,
                                 keep_samples, info, quantiles)
            for le, e in enumerate(mine):
                outs[e] = _element_output(got, le, picks[le], templates[e], delta, B, method, n_win, n_fun, pointwise,
                                          keep_samples)
                if method == 'parametric':
                    chi2 = np.full(n_tot, np.nan)
                    for k in range(n_tot):
                        if picks[le, k] >= 0:
                            chi2[k] = sols[le * n_tot + k]['chi2'][picks[le, k]]
                    outs[e]['chi2_scans'] = chi2
                if got['left_out'][le]:
                    info['left_out'][e] = got['left_out'][le]
    finally:
        for entry in begun:
            if entry[3] is not None:            # (something failed before this launch was waited for: end it, it holds its solver)
                try:
                    entry[3]()
                except Exception:
                    pass
            entry[1]._lock.release()
    return outs, info


def check_quantiles(quantiles, method, n_res):
    """``quantiles=`` of the resampling drivers -> a float array or None; refused before anything is launched"""
    if quantiles is None:
        return None
    if method == 'jackknife':
        raise ValueError("quantiles need method='bootstrap': jackknife pseudo-values are not a sample of the distribution")
    q = np.array(quantiles, dtype=float, ndmin=1)
    if q.ndim != 1 or len(q) < 1 or not np.all((q >= 0.0) & (q <= 1.0)):
        raise ValueError('quantiles={!r}: probabilities in [0, 1] are needed'.format(quantiles))
    if n_res is not None and n_res > device.QUANTILE_MAX_ROWS:
        raise ValueError('quantiles: {} resamples; mxe_resample_quantiles sorts at most {} rows of a group'.format(
            n_res, device.QUANTILE_MAX_ROWS))
    return q


def _host_quantiles(values, q):
    """type-7 quantiles over the finite rows of ``values`` (rows, n) -> (n_q, n); NaN without a finite row"""
    v = np.asarray(values, dtype=float)
    v = v[np.all(np.isfinite(v), axis=1)]
    if len(v) == 0:
        return np.full((len(q), values.shape[1]), np.nan)
    return np.quantile(v, q, axis=0)


def _reduce_device(ctx, picks, n_alpha, method, rows, B, pointwise, keep_samples, info, quantiles=None):
    """``mxe_resample_reduce`` over the elements of one device: per element a group of its resamples (chains 1 ..) at their
    alphas and a group of the full-sample chain alone, whose 'mean' is its H row"""
    n_e, n_tot = picks.shape
    n_res = n_tot - 1
    n_f = len(rows)
    off, prob, members = [0], [], []
    for le in range(n_e):
        mem = [k for k in range(1, n_tot) if picks[le, k] >= 0]
        members.append(mem)
        prob.extend((le * n_tot + k) * n_alpha + int(picks[le, k]) for k in mem)
        off.append(len(prob))
        if picks[le, 0] >= 0:
            prob.append((le * n_tot) * n_alpha + int(picks[le, 0]))
        off.append(len(prob))
    scale = np.ones(2 * n_e)
    for le in range(n_e):
        scale[2 * le] = spread_scale(method, len(members[le]))
    t = {}
    red = ctx.resample_reduce(off, scale, problem_index=prob, F=rows if n_f else None, timing=t)
    info['reduce_ms'] += t.get('ms', 0.0)
    info['reduce_launches'] += 1
    used = red['used'][0::2].copy()
    left_out = [[k - 1 for k in range(1, n_tot) if picks[le, k] < 0] for le in range(n_e)]
    short = [le for le in range(n_e) if used[le] != len(members[le])]
    fix = np.ones(n_e)
    if short:
        # some chosen rows are not finite (an alpha that failed): which ones -- every row as a group of its own, nothing but the
        # counts comes back -- and the scale of the rows that were used
        solo = ctx.resample_reduce(np.arange(len(prob) + 1), np.ones(len(prob)), problem_index=prob, want=(), timing=t)
        info['reduce_ms'] += t.get('ms', 0.0)
        info['reduce_launches'] += 1
        for le in short:
            flags = solo['used'][off[2 * le]:off[2 * le + 1]]
            left_out[le] = sorted(left_out[le] + [k - 1 for k, ok in zip(members[le], flags) if not ok])
            fix[le] = spread_scale(method, used[le]) / scale[2 * le]
    out = dict(used=used, left_out=left_out, members=members, off=off, prob=prob,
               mean=red['mean'][0::2], var=red['var'][0::2] * fix[:, None], H_full=red['mean'][1::2],
               fmean=red['fmean'][0::2], fcov=red['fcov'][0::2] * fix[:, None, None], f_full=red['fmean'][1::2],
               fval=red['fval'])
    if pointwise and B is not None:
        # A = B H: the rows of B as functionals, a chunk at a time (the covariance block of a chunk is formed and dropped)
        Bm = np.asarray(B, dtype=float)
        nw = Bm.shape[0]
        A_mean, A_var, A_full = np.empty((n_e, nw)), np.empty((n_e, nw)), np.empty((n_e, nw))
        for c0 in range(0, nw, BLUR_CHUNK):
            c1 = min(c0 + BLUR_CHUNK, nw)
            part = ctx.resample_reduce(off, scale, problem_index=prob, F=Bm[c0:c1], want=('fmean', 'fcov'), timing=t)
            info['reduce_ms'] += t.get('ms', 0.0)
            info['reduce_launches'] += 1
            A_mean[:, c0:c1] = part['fmean'][0::2]
            A_full[:, c0:c1] = part['fmean'][1::2]
            A_var[:, c0:c1] = np.diagonal(part['fcov'][0::2], axis1=1, axis2=2) * fix[:, None]
        out.update(A_mean=A_mean, A_var=A_var, A_full=A_full)
    if quantiles is not None:
        if pointwise and B is None:
            qs = ctx.resample_quantiles(off, quantiles, problem_index=prob, timing=t)
            info['reduce_ms'] += t.get('ms', 0.0)
            info['reduce_launches'] += 1
            if not np.array_equal(qs['used'][0::2], used):
                raise RuntimeError('resample_errors: mxe_resample_quantiles and mxe_resample_reduce used different rows')
            out['H_q'] = qs['q'][0::2]
        elif pointwise:
            # A = B H: the values of a chunk of rows of B on every resample, their quantiles on the host
            A_q = np.empty((n_e, len(quantiles), nw))
            for c0 in range(0, nw, BLUR_CHUNK):
                c1 = min(c0 + BLUR_CHUNK, nw)
                part = ctx.resample_reduce(off, scale, problem_index=prob, F=Bm[c0:c1], want=('fval',), timing=t)
                info['reduce_ms'] += t.get('ms', 0.0)
                info['reduce_launches'] += 1
                for le in range(n_e):
                    A_q[le, :, c0:c1] = _host_quantiles(part['fval'][off[2 * le]:off[2 * le + 1]], quantiles)
            out['A_q'] = A_q
        if n_f:
            out['f_q'] = np.stack([_host_quantiles(red['fval'][off[2 * le]:off[2 * le + 1]], quantiles) for le in range(n_e)])
        out['quantiles'] = quantiles
    if keep_samples:
        # (asked for: the chosen rows of the resamples come to the host)
        safe = np.where(picks[:, 1:] >= 0, picks[:, 1:], 0)
        want = ((np.arange(n_e)[:, None] * n_tot + np.arange(1, n_tot)[None, :]) * n_alpha + safe).ravel()
        H = ctx.fetch_rows(want).reshape(n_e, n_res, -1)
        H[picks[:, 1:] < 0] = np.nan
        out['samples_H'] = H
    return out


def _element_output(got, le, picks, spec, delta, B, method, n_win, n_fun, pointwise, keep_samples):
    n_res = len(picks) - 1
    n_u = int(got['used'][le])
    i0 = int(picks[0])
    alpha = np.asarray(spec['alpha'], dtype=float)
    out = dict(alpha_index=i0, alpha=float(alpha[i0]) if i0 >= 0 else np.nan,
               alpha_index_samples=np.array(picks[1:], dtype=np.int64), n_used=n_u, n_resamples=n_res, method=method)
    H_full = got['H_full'][le]
    if B is None:
        out['A'] = H_full / delta
    elif 'A_full' in got:
        out['A'] = got['A_full'][le]
    else:
        out['A'] = np.dot(np.asarray(B, dtype=float), H_full)
    if pointwise:
        if B is None:
            out['A_mean'], out['A_err'] = got['mean'][le] / delta, np.sqrt(got['var'][le]) / delta
        else:
            out['A_mean'], out['A_err'] = got['A_mean'][le], np.sqrt(got['A_var'][le])
        if method == 'jackknife':
            out['A_bias'] = (n_u - 1) * (out['A_mean'] - out['A'])
        if 'quantiles' in got:
            out['A_quantiles'] = got['H_q'][le] / delta if B is None else got['A_q'][le]
    if 'quantiles' in got:
        out['quantiles'] = np.array(got['quantiles'])
    nf = n_win + n_fun
    if nf:
        fmean, fcov, ffull = got['fmean'][le], got['fcov'][le], got['f_full'][le]
        ferr = np.sqrt(np.diagonal(fcov))
        if n_win:
            out['window_weight'], out['window_err'], out['window_full'] = fmean[:n_win], ferr[:n_win], ffull[:n_win]
        if n_fun:
            out['functional_value'], out['functional_err'] = fmean[n_win:], ferr[n_win:]
            out['functional_cov'], out['functional_full'] = fcov[n_win:, n_win:], ffull[n_win:]
        if 'f_q' in got:
            if n_win:
                out['window_quantiles'] = got['f_q'][le][:, :n_win]
            if n_fun:
                out['functional_quantiles'] = got['f_q'][le][:, n_win:]
    if keep_samples:
        fun = np.full((n_res, nf), np.nan)
        mem = got['members'][le]
        r0 = got['off'][2 * le]
        for n, k in enumerate(mem):
            fun[k - 1] = got['fval'][r0 + n]
        out['samples'] = dict(H=got['samples_H'][le], functional=fun)
    return out


# ---- TauMaxEnt ---------------------------------------------------------------------------------------------------------

def _stacked_single(tm, bins, who='resample_errors'):
    """``bins`` as the real (n_bins, n_data) sets ``set_G_tau_bins`` / ``set_G_iw_bins`` send down; ``who``: the caller an
    error message names"""
    b = np.asarray(bins)
    if b.ndim != 2:
        raise ValueError('{}: bins must be (n_bins, n_points); their shape is {}'.format(who, b.shape))
    if getattr(tm._inner_kernel(), 'kind', None) == 'iomega':           # (set_G_iw_bins: the only complex bins there are)
        from .kernels import stack_complex
        return np.ascontiguousarray(stack_complex(b), dtype=float)
    if np.iscomplexobj(b):
        raise ValueError('{}: G(tau) bins must be real'.format(who))
    return np.ascontiguousarray(b, dtype=float)


def tau_resample_errors(tm, bins, method='jackknife', block=1, n_resamples=None, seed=None, alpha=None,
                        alpha_mode='per_resample', windows=None, functionals=None, pointwise=True, keep_samples=False,
                        timing=None, quantiles=None):
    quantiles = check_quantiles(quantiles, method, None)
    st = tm.__dict__.get('bin_statistics')
    if st is None:
        raise ValueError('resample_errors: no bins were set; call set_G_tau_bins or set_G_iw_bins first')
    loop = tm.maxent_loop
    check_minimizer(loop)
    stacked = _stacked_single(tm, bins)
    n_data = len(st['mean'])
    if stacked.shape != (st['n_bins'], n_data):
        raise ValueError('resample_errors: bins of shape {} are not those of the last set_G_*_bins call ({} bins of {} '
                         'values)'.format(np.shape(bins), st['n_bins'], n_data))
    if tm.K.rotation is None or loop.err is None or len(loop.err) != st['rank']:
        raise ValueError('resample_errors: the object no longer holds the job of its bins (errors or data were set since)')
    counts = resample_counts(method, st['n_bins'], block, n_resamples, seed)
    t = {}
    got = device.bins_resample(stacked, counts, padded_T(st, n_data), st['rank'], device=tm._device_for_bins(),
                               want_dev=False, timing=t)
    if got['mean'].tobytes() != np.ascontiguousarray(st['mean'], dtype=float).tobytes():
        raise ValueError('resample_errors: these are not the bins of the last set_G_*_bins call (their mean differs)')
    template = loop.make_spec()
    ids = loop.device_ids if loop.device_ids else (loop.device_id,)
    outs, info = element_resamples(tm.K, tm.omega, loop, [template], [got['G'][:, :st['rank']]], method, alpha=alpha,
                                   alpha_mode=alpha_mode, windows=windows, functionals=functionals, pointwise=pointwise,
                                   keep_samples=keep_samples, device_ids=ids[:1], quantiles=quantiles)
    info['resample_ms'] = t.get('ms', 0.0)
    info['left_out'] = info['left_out'].get(0, [])
    out = outs[0]
    out['info'] = info
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['reduce_ms'] + info['resample_ms'], kernel_ms=info['kernel_ms'],
                      reduce_ms=info['reduce_ms'], resample_ms=info['resample_ms'])
    return out


# ---- ElementwiseMaxEnt / DiagonalMaxEnt --------------------------------------------------------------------------------

def _sets_of(ew, bins, who='resample_errors'):
    """the real sets of element (i, j) as ``ElementwiseMaxEnt.set_G_tau_bins`` / ``set_G_iw_bins`` form them; ``who``: the
    caller an error message names"""
    n_iw = ew.__dict__.get('_n_iw')
    if n_iw is None:
        cplx = np.iscomplexobj(bins)
        if cplx and not ew.use_complex:
            raise ValueError('{}: complex G(tau) bins need use_complex=True'.format(who))

        def sets_of(i, j):
            b = bins[:, i, j, :]
            return b.real, (b.imag if cplx else None)
        return sets_of

    def sets_of(i, j):
        a, b = bins[:, i, j, :], bins[:, j, i, :]
        re_part = 0.5 * (a + b)
        re_set = np.concatenate([re_part.real, re_part.imag], axis=-1)
        if not ew.use_complex or i == j:
            return re_set, None
        im_part = (a - b) / 2j
        return re_set, np.concatenate([im_part.real, im_part.imag], axis=-1)
    return sets_of


def elementwise_resample_errors(ew, bins, method='jackknife', block=1, n_resamples=None, seed=None, alpha=None,
                                alpha_mode='per_resample', windows=None, functionals=None, pointwise=True,
                                keep_samples=False, timing=None, quantiles=None):
    from .elementwise_maxent import DiagonalMaxEnt
    quantiles = check_quantiles(quantiles, method, None)
    # a mirrored imaginary part is minus its partner: its quantile q is minus the partner's quantile 1 - q
    mirror = quantiles is not None and ew.use_complex and ew.use_hermiticity and not isinstance(ew, DiagonalMaxEnt)
    n_q = 0 if quantiles is None else len(quantiles)
    q_dev = np.concatenate([quantiles, 1.0 - quantiles]) if mirror else quantiles
    if not ew.__dict__.get('_errors_from_bins') or ew.__dict__.get('bin_statistics') is None:
        raise ValueError('resample_errors: no bins were set; call set_G_tau_bins or set_G_iw_bins first')
    for worker in (ew.maxent_diagonal, ew.maxent_offdiagonal):
        check_minimizer(worker.maxent_loop)
    table = ew.error                                    # {(i, j): [statistics of the real part, of the imaginary part or None]}
    public = ew.bin_statistics
    n_bins = next(iter(public.values()))['n_bins']
    n_data = len(next(iter(public.values()))['mean'])
    bins = np.asarray(bins)
    M, N = ew.shape
    n_iw = ew.__dict__.get('_n_iw')
    n_grid = n_data // 2 if n_iw is not None else n_data
    if bins.ndim != 4 or bins.shape != (n_bins, M, N, n_grid):
        raise ValueError('resample_errors: bins of shape {} are not those of the last set_G_*_bins call {}'.format(
            bins.shape, (n_bins, M, N, n_grid)))
    sets_of = _sets_of(ew, bins)
    where, sets, T, rank = {}, [], [], []
    for (i, j), pair in table.items():
        parts = sets_of(i, j)
        for c in (0, 1):
            if pair[c] is None or parts[c] is None:
                continue
            where[(i, j, c)] = len(sets)
            sets.append(parts[c])
            T.append(padded_T(pair[c], n_data))
            rank.append(pair[c]['rank'])
    if not sets:
        raise ValueError('resample_errors: no element has data')
    counts = resample_counts(method, n_bins, block, n_resamples, seed)
    ids = ew.device_ids if ew.device_ids else (ew.maxent_diagonal._device_for_bins(),)
    t = {}
    got = device.bins_resample(np.ascontiguousarray(np.stack(sets), dtype=float), counts, np.stack(T), rank, device=ids[0],
                               want_dev=False, timing=t)
    for (i, j, c), s in where.items():
        if got['mean'][s].tobytes() != np.ascontiguousarray(table[(i, j)][c]['mean'], dtype=float).tobytes():
            raise ValueError('resample_errors: these are not the bins of the last set_G_*_bins call (the mean of element '
                             '{} {} differs)'.format(i, j))
    phases = [(ew.maxent_diagonal, ew._diag_jobs())]
    if not isinstance(ew, DiagonalMaxEnt):
        phases.append((ew.maxent_offdiagonal, ew._offdiag_jobs()))
    collected = []
    info = dict(kernel_ms=0.0, reduce_ms=0.0, resample_ms=t.get('ms', 0.0), launches=0, reduce_launches=0, n_datasets=[],
                n_elements=[], left_out={})
    for worker, jobs in phases:
        loop = worker.maxent_loop
        templates, G_rows, keys = [], [], []
        for element, re in jobs:
            i, j = element
            c = 0 if (re or i == j) else 1
            s = where.get((i, j, c))
            if s is None:
                continue
            ew._load_element(worker, element, re)
            if loop.below_threshold():
                continue
            templates.append(loop.make_spec())
            G_rows.append(got['G'][s][:, :rank[s]])
            keys.append(tuple(element) + (((0 if re else 1),) if ew.use_complex else ()))
        if not templates:
            continue
        outs, pinfo = element_resamples(worker.K, worker.omega, loop, templates, G_rows, method, alpha=alpha,
                                        alpha_mode=alpha_mode, windows=windows, functionals=functionals,
                                        pointwise=pointwise, keep_samples=keep_samples, device_ids=ids, quantiles=q_dev)
        info['kernel_ms'] += pinfo['kernel_ms']
        info['reduce_ms'] += pinfo['reduce_ms']
        info['launches'] += pinfo['launches']
        info['reduce_launches'] += pinfo['reduce_launches']
        info['n_datasets'].append(pinfo['n_datasets'])
        info['n_elements'].append(len(templates))
        for k in ('audit_max',):
            if k in pinfo:
                info[k] = max(info.get(k, 0.0), pinfo[k])
        for e, lo in pinfo['left_out'].items():
            info['left_out'][keys[e]] = lo
        collected.extend(zip(keys, outs))
    if not collected:
        raise ValueError('resample_errors: every element is below the threshold')
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['reduce_ms'] + info['resample_ms'], kernel_ms=info['kernel_ms'],
                      reduce_ms=info['reduce_ms'], resample_ms=info['resample_ms'])
    out = dict(info=info, method=method, n_resamples=len(counts) - 1)
    if quantiles is not None:
        out['quantiles'] = np.array(quantiles)
    return assemble_elements(ew, collected, out, n_q, mirror)


#: what changes sign in the imaginary part of a hermitian partner, and what is a quantile band (it changes sign AND goes to 1 - q)
SIGNED = ('window_weight', 'window_full', 'functional_value', 'functional_full', 'A', 'A_mean', 'A_bias')
BANDS = ('A_quantiles', 'window_quantiles', 'functional_quantiles')


def assemble_elements(ew, collected, out, n_q=0, mirror=False, shared=('method', 'n_resamples', 'quantiles'), signed=SIGNED):
    """The per-element dicts ``collected`` ((key, dict) pairs) into ``out`` in the layout of
    ``ElementwiseMaxEnt.posterior_errors``: matrix indices, then the complex index with ``use_complex``; NaN (-1 for
    integers) where nothing was computed, the hermitian partners filled in.  The names ``shared`` are the caller's.  A band
    holds ``n_q`` quantiles and, with ``mirror``, behind them the quantiles at 1 - q, which -- with the other sign -- are
    the quantiles of a mirrored imaginary part."""
    struct = tuple(ew.shape) + ((2,) if ew.use_complex else ())
    for key, o in collected:
        partner = (key[1], key[0]) + key[2:] if (ew.use_hermiticity and key[0] != key[1]) else None
        # G_ji = conj(G_ij): the same errors; the imaginary part's values change sign
        flip = -1.0 if (len(key) == 3 and key[2] == 1) else 1.0
        for name, val in o.items():
            if name in shared:
                continue
            if name in BANDS:
                val = np.asarray(val)
                if name not in out:
                    out[name] = np.full(struct + (n_q,) + val.shape[1:], np.nan)
                out[name][key] = val[:n_q]
                if partner is not None:
                    out[name][partner] = -val[n_q:] if (mirror and flip < 0) else val[:n_q]
                continue
            if name == 'samples':
                held = out.setdefault('samples', {})
                for sub, arr in val.items():
                    if sub not in held:
                        held[sub] = np.full(struct + arr.shape, np.nan)
                    held[sub][key] = arr
                    if partner is not None:
                        held[sub][partner] = arr * flip
                continue
            val = np.asarray(val)
            if name not in out:
                out[name] = np.full(struct + val.shape, np.nan) if val.dtype.kind == 'f' else \
                    np.full(struct + val.shape, -1, dtype=val.dtype)
            out[name][key] = val
            if partner is not None:
                out[name][partner] = val * flip if (val.dtype.kind == 'f' and name in signed) else val
    return out
