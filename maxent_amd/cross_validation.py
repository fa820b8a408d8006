"""k-fold cross-validation of alpha over Monte Carlo bins (``TauMaxEnt.cross_validate``,
``ElementwiseMaxEnt.cross_validate``, :func:`cross_validation_score`).  Not in the reference, which has no bins.

The one question that needs no approximation: does the spectrum continued from one part of the Monte Carlo data predict
the other part?  The bins are independent noise realisations of the same G, so BINS are split, not tau points (the rows
of K are nearly collinear: a held-out tau point tests almost nothing).  The bins are cut into K contiguous folds -- the
bin index is Monte Carlo time, contiguous folds keep autocorrelated neighbours on one side of the split --; for every
fold the mean of the other bins is continued over the whole alpha mesh, and every H row of that scan is scored against
the mean of the fold,

    chi2_val(f, alpha) = sum_{k < rank} w[f][k] ((T K H_{f, alpha})[k] - (T mean_f)[k])^2,   w[f][k] = N_f / (N sigma_k^2),

in the eigenbasis T of the full-sample covariance; sigma_k^2 is the variance of the full-sample mean along direction k
(``bin_statistics['sigma']``), N the number of bins, N_f the size of the fold: w is the inverse variance of the mean of
N_f independent bins.  The score falls with alpha while the fit still learns signal and rises once it learns the noise
of its training part.

What is approximate.  (1) The training solve at mesh alpha uses the full-sample sigma and T -- the element's ONE data set
on the device, as ``set_G_*_bins`` staged it, shrinkage included.  A training mean of N - N_f bins is noisier by
N / (N - N_f), so the solve equals one with the training mean's own error at alpha (N - N_f) / N
(``info['alpha_train_factor']``, the mean over the folds).  The pick is applied to the full sample at the same mesh index,
the plug-in rule.  (2) sigma and T are estimated from all bins, the validation fold included.  (3) K-fold with few bins per
fold is noisy; ``score_err`` says how noisy, and the one-standard-error rule (the largest alpha whose score is within
``score_err`` of the minimum) is the usual guard.

The 1 + K scans of every element are one launch of the solver per device, and one ``mxe_cv_score`` call per device then
reads the K n_alpha training rows of every element where they lie: no H row of a fold crosses to the host.  This module
is the host glue: the table of folds, the weights, the pick rules, the shape of what is returned.  There is no CPU path.
"""

import numpy as np

from . import device

NAME = 'CrossValidationAnalyzer'
RULES = ('min', 'one_se')


# ---- folds and pick rules (no device) ----------------------------------------------------------------------------------

def fold_ranges(n_bins, n_folds):
    """the K contiguous ranges of bins [(start, stop), ...]; their sizes differ by at most one, the longer ones first"""
    n_bins, n_folds = int(n_bins), int(n_folds)
    if n_folds < 2 or 2 * n_folds > n_bins:
        raise ValueError('cross-validation: {} folds of {} bins (at least 2 folds of at least 2 bins are needed)'.format(
            n_folds, n_bins))
    base, extra = divmod(n_bins, n_folds)
    edges = [f * base + min(f, extra) for f in range(n_folds + 1)]
    return [(edges[f], edges[f + 1]) for f in range(n_folds)]


def fold_counts(n_bins, n_folds):
    """the table ``mxe_bins_resample`` takes, 1 + 2 K rows of n_bins multiplicities: the full sample (ones), the K
    training rows (0 inside fold f, 1 outside), the K validation rows (1 inside fold f, 0 outside).  The folds are K
    contiguous ranges of bins whose sizes differ by at most one.  ``ValueError`` unless 2 <= K and 2 K <= n_bins."""
    ranges = fold_ranges(n_bins, n_folds)
    K = len(ranges)
    counts = np.ones((1 + 2 * K, int(n_bins)), dtype=np.int32)
    for f, (a, b) in enumerate(ranges):
        counts[1 + f, a:b] = 0
        counts[1 + K + f] = 0
        counts[1 + K + f, a:b] = 1
    return counts


def pick(alpha, fold_scores):
    """The rules on a table ``fold_scores`` (K, n_alpha): a dict with ``score`` (the mean over the folds), ``score_err``
    (their standard deviation / sqrt(K)) -- NaN at an alpha where a fold is not finite --, ``alpha_index_cv`` (the argmin
    of ``score``; of equal scores the larger alpha; -1 when no alpha has all its folds), ``alpha_index_one_se`` (the
    largest alpha whose score is <= the minimum + ``score_err`` at the minimum) and ``alpha_at_edge`` (the minimum sits on
    an end of the mesh)."""
    alpha = np.asarray(alpha, dtype=float)
    fs = np.atleast_2d(np.asarray(fold_scores, dtype=float))
    K = fs.shape[0]
    ok = np.all(np.isfinite(fs), axis=0)
    score, err = np.full(fs.shape[1], np.nan), np.full(fs.shape[1], np.nan)
    if np.any(ok):
        score[ok] = np.mean(fs[:, ok], axis=0)
        err[ok] = (np.std(fs[:, ok], axis=0, ddof=1) if K > 1 else 0.0) / np.sqrt(K)
    out = dict(score=score, score_err=err, alpha_index_cv=-1, alpha_index_one_se=-1, alpha_at_edge=False)
    if not np.any(ok):
        return out
    idx = np.flatnonzero(ok)
    best = score[idx].min()
    i_cv = int(max(idx[score[idx] == best], key=lambda i: alpha[i]))
    within = idx[score[idx] <= best + err[i_cv]]
    out['alpha_index_cv'] = i_cv
    out['alpha_index_one_se'] = int(max(within, key=lambda i: alpha[i]))
    out['alpha_at_edge'] = bool(i_cv in (0, len(alpha) - 1))
    return out


def fold_weights(sigma, n_bins, ranges):
    """``w[f][k] = N_f / (N sigma_k^2)``: the inverse variance of the mean of the N_f bins of fold f along direction k"""
    s2 = np.asarray(sigma, dtype=float) ** 2
    return np.stack([(b - a) / (float(n_bins) * s2) for a, b in ranges])


# ---- the plain function --------------------------------------------------------------------------------------------------

def cross_validation_score(H, K, Gval, w, T=None, rank=None, device=0):
    """``mxe_cv_score`` for H rows from anywhere.  ``H``: (n_groups, rows, n_omega), or (rows, n_omega) for one group;
    ``K``: (n_data, n_omega), the kernel that acts on H, not rotated; ``Gval``, ``w``: (n_groups, n_data) held-out data in
    the basis ``T`` and weights >= 0; ``T``, ``rank``: (n_groups, n_data, n_data) and (n_groups,) as ``mxe_bins_eig`` gives
    them (zero rows behind the rank), or both None: the identity.  Returns a dict: ``z`` (n_groups, rows, n_data) with
    ``z = sqrt(w) (T K H - Gval)`` for k < rank and 0 behind it, ``score`` (n_groups, rows) = sum_k z^2 -- NaN for a row
    of H that is not finite --, ``used`` (n_groups: finite rows), ``ms`` (the device time)."""
    H = np.asarray(H, dtype=float)
    single = H.ndim == 2
    if single:
        H = H[np.newaxis]
    if H.ndim != 3:
        raise ValueError('cross_validation_score: H must be (n_groups, rows, n_omega) or (rows, n_omega), got {}'.format(H.shape))
    ng, rows, n_omega = H.shape
    K = np.atleast_2d(np.asarray(K, dtype=float))
    if K.shape[1] != n_omega:
        raise ValueError('cross_validation_score: K has {} columns, H {} points'.format(K.shape[1], n_omega))
    n_data = K.shape[0]
    Gval, w = np.asarray(Gval, dtype=float).reshape(-1, n_data), np.asarray(w, dtype=float).reshape(-1, n_data)
    if T is not None:
        T = np.asarray(T, dtype=float).reshape(-1, n_data, n_data)
    ctx = device_context(n_omega, device)
    try:
        t = {}
        got = ctx.cv_score(np.arange(ng + 1) * rows, K, Gval, w, T=T, rank=rank, H=H.reshape(ng * rows, n_omega), timing=t)
    finally:
        ctx.close()
    out = dict(z=got['z'].reshape(ng, rows, n_data), score=got['score'].reshape(ng, rows), used=got['used'], ms=t.get('ms', 0.0))
    if single:
        out = dict((k, v[0] if k != 'ms' else v) for k, v in out.items())
    return out


def device_context(n_omega, device_id=0):
    """a context that holds no kernel of a job: all ``mxe_cv_score`` needs when the H rows are handed in"""
    return device.DeviceContext(None, np.ones(1), np.ones((int(n_omega), 1)), device=device_id)


# ---- the device part: the scans of the folds of several elements of one kernel --------------------------------------------

def element_cross_validation(K, omega, loop, templates, G_rows, G_val, weights, T, rank, ranges, n_bins, device_ids=None,
                             keep_rows=False):
    """The cross-validation of the elements ``templates`` (their specs, as ``MaxEntLoop.make_spec`` makes them) of one
    kernel.  ``G_rows[e]``: (1 + K, rank_e) rotated data of element e, row 0 the full sample, rows 1 .. the training means;
    ``G_val[e]``, ``weights[e]``: (K, n_data) validation means in the rotated basis and their weights; ``T[e]``
    (n_data, n_data, zero rows behind the rank), ``rank[e]``.  Element e is solved on device e mod N -- all its 1 + K scans
    on that device, one launch per device -- and scored there by one ``mxe_cv_score`` call over the K n_alpha training rows
    of every element, read where they lie.  Returns (list of dicts, one per element, info)."""
    from .batch_solver import BatchSolver, directions_to_keep
    from .maxent_loop import solve_elements
    from .mock import unrotated_matrix
    from .resampling import check_minimizer
    check_minimizer(loop)
    delta = np.asarray(omega.delta, dtype=float)
    n_elem, n_tot = len(templates), int(G_rows[0].shape[0])
    Kf = n_tot - 1
    n_alpha = len(templates[0]['alpha'])
    Ku = np.ascontiguousarray(unrotated_matrix(K))
    n_data = Ku.shape[0]
    B = loop.A_of_H.matrix()
    ids = tuple(device_ids) if device_ids else (loop.device_id,)
    N = len(ids)
    per_dev = [[e for e in range(n_elem) if e % N == r] for r in range(N)]
    outs = [None] * n_elem
    sizes = np.array([b - a for a, b in ranges], dtype=float)
    info = dict(kernel_ms=0.0, score_ms=0.0, launches=0, score_launches=0, devices=[],
                alpha_train_factor=float(np.mean((n_bins - sizes) / n_bins)))
    begun = []
    try:
        for r, dev in enumerate(ids):
            if not per_dev[r]:
                continue
            specs = [loop.spec_like(templates[e], G_rows[e][k], templates[e]['err']) for e in per_dev[r] for k in range(n_tot)]
            solver = BatchSolver.for_kernel(K, (dev,), keep=directions_to_keep(K, specs, None, chi2_factor=loop.cost_function.chi2_factor))
            solver._lock.acquire()              # (until this device's rows are scored: nobody else launches on its contexts)
            begun.append([r, solver, specs, None])
            begun[-1][3] = solve_elements(K, specs, loop.minimizer, device_ids=(dev,),
                                          chi2_factor=loop.cost_function.chi2_factor, select=None, want_H=False, defer=True)
        for entry in begun:
            r, solver, specs, end = entry
            entry[3] = None
            sols, launch = end()
            if solver.last_info is not launch:
                raise RuntimeError('cross_validate: the launch ran on another solver than the one that was locked')
            info['kernel_ms'] = max(info['kernel_ms'], launch.get('kernel_ms', 0.0))
            info['launches'] += 1
            info['devices'].append(ids[r])
            for k in ('audit_max', 'audit_problems'):
                if k in launch:
                    info[k] = max(info.get(k, 0.0), launch[k]) if k == 'audit_max' else info.get(k, 0) + launch[k]
            mine = per_dev[r]
            ctx = solver.ctxs[0]
            # group (element, fold): the n_alpha rows of chain le n_tot + 1 + f
            chains = (np.arange(len(mine))[:, None] * n_tot + 1 + np.arange(Kf)[None, :]).ravel()
            prob = (chains[:, None] * n_alpha + np.arange(n_alpha)[None, :]).ravel()
            off = np.arange(len(chains) + 1) * n_alpha
            Tg = np.repeat(np.stack([T[e] for e in mine]), Kf, axis=0)
            rk = np.repeat(np.array([rank[e] for e in mine], dtype=np.int32), Kf)
            Gv = np.concatenate([G_val[e] for e in mine])
            wg = np.concatenate([weights[e] for e in mine])
            t = {}
            # (z of every row comes back with the scores, rows x n_data doubles -- 2/5 of what the H rows would be at 500
            #  omega points and 200 data values: the picks are known only afterwards, and a second call for the picked rows
            #  alone would upload every rotation a second time)
            got = ctx.cv_score(off, Ku, Gv, wg, T=Tg, rank=rk, problem_index=prob, timing=t)
            info['score_ms'] += t.get('ms', 0.0)
            info['score_launches'] += 1
            scores = got['score'].reshape(len(mine), Kf, n_alpha)
            z = got['z'].reshape(len(mine), Kf, n_alpha, n_data)
            picked, rows_full = [], []
            for le, e in enumerate(mine):
                alpha = np.asarray(templates[e]['alpha'], dtype=float)
                o = dict(alpha=alpha, fold_scores=scores[le] / float(rank[e]))
                o.update(pick(alpha, o['fold_scores']))
                o['train_chi2'] = np.stack([np.asarray(sols[le * n_tot + 1 + f]['chi2'], dtype=float) for f in range(Kf)])
                o['left_out'] = [(int(f), int(a)) for f, a in zip(*np.nonzero(~np.isfinite(o['fold_scores'])))]
                o['folds'] = np.array(ranges, dtype=np.int64)
                picked.append(o)
                for i in (o['alpha_index_cv'], o['alpha_index_one_se']):
                    rows_full.append((le * n_tot) * n_alpha + max(i, 0))
            # the full-sample rows of the picks come to the host
            Hf = ctx.fetch_rows(rows_full).reshape(len(mine), 2, -1)
            if keep_rows:
                Hk = ctx.fetch_rows(prob).reshape(len(mine), Kf, n_alpha, -1)
            for le, e in enumerate(mine):
                o = picked[le]
                for name, slot in (('A_cv', 0), ('A_one_se', 1)):
                    i = o['alpha_index_' + name[2:]]
                    Hrow = Hf[le, slot] if i >= 0 else np.full(len(delta), np.nan)
                    o[name] = Hrow / delta if B is None else np.dot(np.asarray(B, dtype=float), Hrow)
                o['z'] = np.array(z[le, :, o['alpha_index_cv'], :int(rank[e])]) if o['alpha_index_cv'] >= 0 else \
                    np.full((Kf, int(rank[e])), np.nan)
                o['calibration'] = float(np.mean(o['z'] ** 2)) if o['z'].size else np.nan
                if keep_rows:
                    o['rows_H'] = Hk[le]
                outs[e] = o
    finally:
        for entry in begun:
            if entry[3] is not None:            # (something failed before this launch was waited for: end it, it holds its solver)
                try:
                    entry[3]()
                except Exception:
                    pass
            entry[1]._lock.release()
    return outs, info


def check_rule(rule):
    if rule not in RULES:
        raise ValueError("rule={!r}: 'min' or 'one_se'".format(rule))
    return 'alpha_index_cv' if rule == 'min' else 'alpha_index_one_se'


def analyzer_result(o, rule):
    """the entry ``analyzer_results['CrossValidationAnalyzer']`` of one element: ``alpha_index`` and ``A_out`` follow ``rule``"""
    from .analyzers import AnalyzerResult
    idx = int(o[check_rule(rule)])
    res = AnalyzerResult()
    res.update(name=NAME, alpha_index=idx, A_out=np.array(o['A_cv' if rule == 'min' else 'A_one_se']), rule=rule,
               score=np.array(o['score']), score_err=np.array(o['score_err']),
               info='Cross-validated alpha ({}): {} (= index {} zero-based)'.format(
                   rule, o['alpha'][idx] if idx >= 0 else np.nan, idx))
    return res


def attach(result, key, o, rule):
    """add the entry beside those of ``run()``; the default analyzer stays what it was"""
    if int(o[check_rule(rule)]) < 0:
        return
    res = analyzer_result(o, rule)
    res.maxent_result = result
    table = result._analysis
    if key not in table:
        table[key] = {}
    table[key][NAME] = res
    result._cache.pop('analyzer_results', None)


def _fold_data(got_G, st, ranges, n_bins, n_data):
    """of one set: (G_rows (1 + K, rank), G_val (K, n_data), weights (K, n_data): zero behind the rank)"""
    Kf, r = len(ranges), int(st['rank'])
    w = np.zeros((Kf, n_data))
    w[:, :r] = fold_weights(st['sigma'], n_bins, ranges)
    return got_G[:1 + Kf, :r], np.ascontiguousarray(got_G[1 + Kf:]), w


# ---- TauMaxEnt ---------------------------------------------------------------------------------------------------------

def tau_cross_validate(tm, bins, n_folds=5, rule='min', result=None, keep_rows=False, timing=None):
    from . import posterior
    from .resampling import _stacked_single, check_minimizer, padded_T
    check_rule(rule)
    st = tm.__dict__.get('bin_statistics')
    if st is None:
        raise ValueError('cross_validate: no bins were set; call set_G_tau_bins, set_G_iw_bins or set_G_l_bins first')
    loop = tm.maxent_loop
    check_minimizer(loop)
    stacked = _stacked_single(tm, bins, who='cross_validate')
    n_data = len(st['mean'])
    if stacked.shape != (st['n_bins'], n_data):
        raise ValueError('cross_validate: bins of shape {} are not those of the last set_G_*_bins call ({} bins of {} '
                         'values)'.format(np.shape(bins), st['n_bins'], n_data))
    if tm.K.rotation is None or loop.err is None or len(loop.err) != st['rank']:
        raise ValueError('cross_validate: the object no longer holds the job of its bins (errors or data were set since)')
    ranges = fold_ranges(st['n_bins'], n_folds)
    counts = fold_counts(st['n_bins'], n_folds)
    template = loop.make_spec()
    if result is not None:
        try:
            posterior.check_alpha(template, result.alpha)
        except ValueError as e:
            raise ValueError('cross_validate: ' + str(e))
    t = {}
    Tp = padded_T(st, n_data)
    got = device.bins_resample(stacked, counts, Tp, st['rank'], device=tm._device_for_bins(), want_dev=False, timing=t)
    if got['mean'].tobytes() != np.ascontiguousarray(st['mean'], dtype=float).tobytes():
        raise ValueError('cross_validate: these are not the bins of the last set_G_*_bins call (their mean differs)')
    G_rows, G_val, w = _fold_data(got['G'], st, ranges, st['n_bins'], n_data)
    ids = loop.device_ids if loop.device_ids else (loop.device_id,)
    outs, info = element_cross_validation(tm.K, tm.omega, loop, [template], [G_rows], [G_val], [w], [Tp], [st['rank']], ranges,
                                          st['n_bins'], device_ids=ids[:1], keep_rows=keep_rows)
    info['resample_ms'] = t.get('ms', 0.0)
    out = outs[0]
    out.update(info=info, rule=rule, n_folds=len(ranges))
    if result is not None:
        attach(result, None, out, rule)
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['score_ms'] + info['resample_ms'], kernel_ms=info['kernel_ms'],
                      score_ms=info['score_ms'], resample_ms=info['resample_ms'])
    return out


# ---- ElementwiseMaxEnt / DiagonalMaxEnt --------------------------------------------------------------------------------

#: what changes sign in the imaginary part of a hermitian partner
SIGNED = ('A_cv', 'A_one_se')


def elementwise_cross_validate(ew, bins, n_folds=5, rule='min', result=None, keep_rows=False, timing=None):
    from . import posterior
    from .elementwise_maxent import DiagonalMaxEnt
    from .resampling import _sets_of, assemble_elements, check_minimizer, padded_T
    check_rule(rule)
    if not ew.__dict__.get('_errors_from_bins') or ew.__dict__.get('bin_statistics') is None:
        raise ValueError('cross_validate: no bins were set; call set_G_tau_bins or set_G_iw_bins first')
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
        raise ValueError('cross_validate: bins of shape {} are not those of the last set_G_*_bins call {}'.format(
            bins.shape, (n_bins, M, N, n_grid)))
    sets_of = _sets_of(ew, bins, who='cross_validate')
    ranges = fold_ranges(n_bins, n_folds)
    counts = fold_counts(n_bins, n_folds)
    where, sets, T, rank, stats = {}, [], [], [], []
    for (i, j), pair in table.items():
        parts = sets_of(i, j)
        for c in (0, 1):
            if pair[c] is None or parts[c] is None:
                continue
            where[(i, j, c)] = len(sets)
            sets.append(parts[c])
            T.append(padded_T(pair[c], n_data))
            rank.append(pair[c]['rank'])
            stats.append(pair[c])
    if not sets:
        raise ValueError('cross_validate: no element has data')
    phases = [(ew.maxent_diagonal, ew._diag_jobs())]
    if not isinstance(ew, DiagonalMaxEnt):
        phases.append((ew.maxent_offdiagonal, ew._offdiag_jobs()))
    if result is not None:
        # (before anything is asked of the device: the mesh up to its scale, which is the element's; every element is
        #  checked against its own spec below)
        theirs = np.asarray(result.alpha, dtype=float)
        for worker, jobs in phases:
            mesh = np.asarray(worker.maxent_loop.alpha_mesh, dtype=float)
            if mesh.shape != theirs.shape or not np.allclose(mesh * theirs[0], theirs * mesh[0], rtol=1e-12, atol=0.0):
                raise ValueError('cross_validate: the alphas of the result are not those of this object (alpha_mesh as it '
                                 'was when the result was made is needed)')
    ids = ew.device_ids if ew.device_ids else (ew.maxent_diagonal._device_for_bins(),)
    t = {}
    got = device.bins_resample(np.ascontiguousarray(np.stack(sets), dtype=float), counts, np.stack(T), rank, device=ids[0],
                               want_dev=False, timing=t)
    for (i, j, c), s in where.items():
        if got['mean'][s].tobytes() != np.ascontiguousarray(table[(i, j)][c]['mean'], dtype=float).tobytes():
            raise ValueError('cross_validate: these are not the bins of the last set_G_*_bins call (the mean of element '
                             '{} {} differs)'.format(i, j))
    collected = []
    info = dict(kernel_ms=0.0, score_ms=0.0, resample_ms=t.get('ms', 0.0), launches=0, score_launches=0, devices=[],
                n_elements=[])
    for worker, jobs in phases:
        loop = worker.maxent_loop
        templates, keys, data, Ts, rks = [], [], [], [], []
        for element, re in jobs:
            i, j = element
            c = 0 if (re or i == j) else 1
            s = where.get((i, j, c))
            if s is None:
                continue
            ew._load_element(worker, element, re)
            if loop.below_threshold():
                continue
            spec = loop.make_spec()
            if result is not None:
                try:
                    posterior.check_alpha(spec, result.alpha)
                except ValueError as e:
                    raise ValueError('cross_validate: ' + str(e))
            templates.append(spec)
            data.append(_fold_data(got['G'][s], stats[s], ranges, n_bins, n_data))
            Ts.append(T[s])
            rks.append(rank[s])
            keys.append(tuple(element) + (((0 if re else 1),) if ew.use_complex else ()))
        if not templates:
            continue
        outs, pinfo = element_cross_validation(worker.K, worker.omega, loop, templates, [d[0] for d in data],
                                               [d[1] for d in data], [d[2] for d in data], Ts, rks, ranges, n_bins,
                                               device_ids=ids, keep_rows=keep_rows)
        for k in ('kernel_ms', 'score_ms', 'launches', 'score_launches'):
            info[k] += pinfo[k]
        info['devices'] = sorted(set(info['devices']) | set(pinfo['devices']))
        info['alpha_train_factor'] = pinfo['alpha_train_factor']
        info['n_elements'].append(len(templates))
        if 'audit_max' in pinfo:
            info['audit_max'] = max(info.get('audit_max', 0.0), pinfo['audit_max'])
        collected.extend(zip(keys, outs))
    if not collected:
        raise ValueError('cross_validate: every element is below the threshold')
    if result is not None:
        for key, o in collected:
            attach(result, key, o, rule)
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['score_ms'] + info['resample_ms'], kernel_ms=info['kernel_ms'],
                      score_ms=info['score_ms'], resample_ms=info['resample_ms'])
    out = dict(info=info, rule=rule, n_folds=len(ranges), folds=np.array(ranges, dtype=np.int64))
    left, edge = {}, {}
    longest = max(int(r) for r in rank)
    for key, o in collected:
        lo = o.pop('left_out')
        if lo:
            left[key] = lo
        o.pop('folds')
        o['z'] = np.pad(o['z'], [(0, 0), (0, longest - o['z'].shape[1])], constant_values=np.nan)
        edge[key] = bool(o.pop('alpha_at_edge'))
    out['left_out'] = left
    out = assemble_elements(ew, collected, out, shared=('rule', 'n_folds', 'folds', 'left_out', 'info'), signed=SIGNED)
    # (a flag: False where nothing was computed, which the integer fill of assemble_elements cannot say)
    out['alpha_at_edge'] = np.zeros(out['alpha_index_cv'].shape, dtype=bool)
    for key, flag in edge.items():
        out['alpha_at_edge'][key] = flag
        if ew.use_hermiticity and key[0] != key[1]:
            out['alpha_at_edge'][(key[1], key[0]) + key[2:]] = flag
    return out
