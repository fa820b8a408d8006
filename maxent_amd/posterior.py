"""Posterior error bars of a MaxEnt result (``TauMaxEnt.posterior_errors``, ``ElementwiseMaxEnt.posterior_errors``).

In the Gaussian approximation around the minimiser of ``Q = eta chi2 / 2 - alpha~ S`` (Bryan 1990; Jarrell &
Gubernatis 1996, section 5) the hidden image H has the covariance

    Gamma = (eta K^T Sigma^-1 K + alpha~ diag(1/w))^-1,     w = H  |  sqrt(H^2 + 4 D^2)  (plus-minus entropy)

with the K, H and alpha~ of this package (``result.G_rec = K H``, ``result.alpha`` is the scaled alpha).  Only
*integrated* quantities have meaningful errors: spectral weight in a window, moments, any ``f^T A delta_omega``.  The
point-wise error ``A_err`` is there for completeness; it is large and strongly correlated between neighbours.

The variances come from ``mxe_posterior_var`` (one call per device for all matrix elements and alphas); this module is
the host glue: which alphas, which rows of weights on H, the mixture over alpha, the shape of what is returned.
There is no CPU path: without the library and a GPU :class:`maxent_amd.device.MaxEntDeviceError` is raised.
"""

import numpy as np

from . import device
from .analyzers import BryanAnalyzer, get_delta


# ---- host glue (no device) ------------------------------------------------------------------------------------------

def window_rows(omega, windows):
    """indicator rows of the windows ``[(lo, hi), ...]`` on the mesh ``omega``: 1 at the points lo <= omega_i <= hi.
    A window must lie inside the mesh and hold at least one point."""
    w = np.asarray(omega, dtype=float)
    rows = np.zeros((len(windows), len(w)))
    for n, win in enumerate(windows):
        if np.shape(win) != (2,):
            raise ValueError('window {}: a pair (omega_lo, omega_hi) is needed, got {!r}'.format(n, win))
        lo, hi = float(win[0]), float(win[1])
        if not (np.isfinite(lo) and np.isfinite(hi)) or not lo < hi:
            raise ValueError('window {}: ({}, {}) is not an interval'.format(n, lo, hi))
        if lo < w.min() or hi > w.max():
            raise ValueError('window {}: ({}, {}) reaches outside the omega mesh [{}, {}]'.format(n, lo, hi, w.min(), w.max()))
        inside = (w >= lo) & (w <= hi)
        if not inside.any():
            raise ValueError('window {}: ({}, {}) holds no point of the omega mesh'.format(n, lo, hi))
        rows[n, inside] = 1.0
    return rows


def functional_rows(functionals, n_omega):
    F = np.atleast_2d(np.asarray(functionals, dtype=float))
    if F.ndim != 2 or F.shape[1] != n_omega:
        raise ValueError('functionals: shape (n_f, n_omega = {}) is needed, got {}'.format(n_omega, np.shape(functionals)))
    if not np.all(np.isfinite(F)):
        raise ValueError('functionals hold values that are not finite')
    return F


def rows_on_H(rows, delta, B=None):
    """weights ``f`` applied to ``A delta_omega`` as weights on the hidden image: ``f`` itself (A delta = H), or with a
    preblur (A = B H) ``B^T (f o delta)``"""
    rows = np.asarray(rows, dtype=float)
    if B is None:
        return rows
    return np.dot(rows * np.asarray(delta, dtype=float)[np.newaxis, :], np.asarray(B, dtype=float))


def bryan_weights(logp, alpha, average_by_integration=False):
    """(mask of the alphas that have a probability, their weights) exactly as ``BryanAnalyzer.analyze`` forms them"""
    logp = np.asarray(logp, dtype=float)
    if np.all(np.isnan(logp)):
        raise ValueError('Probability not calculated. Cannot use BryanAnalyzer.')
    alpha = np.asarray(alpha, dtype=float)
    good = np.logical_not(np.isnan(logp))
    p = np.exp(logp[good] - np.nanmax(logp))
    if average_by_integration:
        p = p / np.trapezoid(p, alpha[good])
        p = p * get_delta(alpha[good])
    else:
        p = p / np.sum(p)
    return good, p


def bryan_mixture(p, values, variances):
    """mean ``sum_a p_a x_a`` and variance ``sum_a p_a [var_a + (x_a - mean)^2]`` of the mixture over alpha;
    ``values``, ``variances``: (n_alpha, ...)"""
    p = np.asarray(p, dtype=float)
    values, variances = np.asarray(values, dtype=float), np.asarray(variances, dtype=float)
    pp = p.reshape((-1,) + (1,) * (values.ndim - 1))
    mean = np.sum(pp * values, axis=0)
    var = np.sum(pp * (variances + (values - mean[np.newaxis]) ** 2), axis=0)
    return mean, var


def choose_alpha(alpha, n_alpha, analysis, default_name):
    """``alpha=`` of posterior_errors -> (indices, reduce) with reduce one of 'one' (the alpha axis is dropped), 'many',
    'bryan'.  ``analysis``: the analyzer results of the element (name -> dict with ``alpha_index``)."""
    if alpha is None:
        alpha = default_name if default_name is not None else 'LineFitAnalyzer'
    if isinstance(alpha, str):
        if alpha == 'all':
            return list(range(n_alpha)), 'many'
        if alpha == 'bryan':
            return list(range(n_alpha)), 'bryan'
        try:
            res = analysis[alpha]
        except (KeyError, TypeError, IndexError):
            raise ValueError('alpha={!r}: the result has no analyzer of this name'.format(alpha))
        idx = res.get('alpha_index') if hasattr(res, 'get') else None
        if idx is None:
            raise ValueError('alpha={!r}: this analyzer chooses no single alpha (no alpha_index)'.format(alpha))
        return [int(idx)], 'one'
    if np.ndim(alpha) == 0:
        idx, how = [int(alpha)], 'one'
    else:
        idx, how = [int(a) for a in alpha], 'many'
        if not idx:
            raise ValueError('alpha: an empty sequence of indices')
    for i in idx:
        if not -n_alpha <= i < n_alpha:
            raise ValueError('alpha index {} out of range for {} alphas'.format(i, n_alpha))
    return [i % n_alpha for i in idx], how


def entropy_weights(H, D, kind):
    """``w = -1 / (d2S/dH2)``: H for the normal entropy, sqrt(H^2 + 4 D^2) for the plus-minus one"""
    H = np.asarray(H, dtype=float)
    if kind == device.ENTROPY_NORMAL:
        return H
    return np.sqrt(H * H + 4.0 * np.asarray(D, dtype=float) ** 2)


# ---- the device part ------------------------------------------------------------------------------------------------

def _stage(K, specs, dev):
    """a context of its own with the elements of ``specs`` (as :class:`maxent_amd.evaluator.Evaluator` stages one)"""
    U, S, V = np.array(K.U), np.array(K.S), np.array(K.V)
    if len(S) > 128:
        raise device.MaxEntDeviceError('posterior errors are computed with at most 128 singular values; call '
                                       'K.reduce_singular_space() first ({} kept now)'.format(len(S)))
    rotated = K.rotation is not None
    ctx = device.DeviceContext(None if rotated else U, S, V, device=dev)
    try:
        ds_ids, seen = [], []
        for s in specs:
            err = np.asarray(s['err'], dtype=float) * np.ones(len(s['G']))
            U_rot = s.get('U_rot')
            found = None
            for (e0, u0, i0) in seen:
                if u0 is U_rot and e0.shape == err.shape and np.array_equal(e0, err):
                    found = i0
                    break
            if found is None:
                found = ctx.add_dataset(err, U if (U_rot is None and rotated) else U_rot)
                seen.append((err, U_rot, found))
            ds_ids.append(found)
        ctx.set_elements(ds_ids, [np.asarray(s['G'], dtype=float) for s in specs],
                         np.stack([np.asarray(s['D'], dtype=float) for s in specs]), [s['kind'] for s in specs])
    except Exception:
        ctx.close()
        raise
    return ctx


def device_variances(K, specs, H_rows, alpha_rows, F, want_diag, chi2_factor=1.0, device_ids=None, timing=None):
    """``mxe_posterior_var`` for the elements ``specs`` of the kernel ``K``: element e with the hidden images
    ``H_rows[e]`` (n_e, n_omega) at ``alpha_rows[e]`` (n_e).  ONE call per device for everything (element e on device
    e mod N, as the solve shards them).  Returns per element ``var``, ``prior`` (n_e, n_f) and ``diag`` (n_e, n_omega) or
    None."""
    device_ids = tuple(device_ids) if device_ids else (0,)
    n = len(specs)
    out_var, out_prior, out_diag = [None] * n, [None] * n, [None] * n
    ms, reused = 0.0, 0
    for r, dev in enumerate(device_ids):
        mine = list(range(r, n, len(device_ids)))
        if not mine:
            continue
        sub = [specs[e] for e in mine]
        from .batch_solver import BatchSolver
        ctx, solver = BatchSolver.staged_context_for(K, sub, dev) if len(device_ids) == 1 else (None, None)
        own = ctx is None
        reused += 0 if own else 1
        if own:
            ctx = _stage(K, sub, dev)
        try:
            el = np.concatenate([np.full(len(alpha_rows[e]), k, dtype=np.int32) for k, e in enumerate(mine)])
            al = np.concatenate([np.asarray(alpha_rows[e], dtype=float) for e in mine])
            Hs = np.concatenate([np.asarray(H_rows[e], dtype=float).reshape(len(alpha_rows[e]), -1) for e in mine])
            t = {}
            if solver is not None:
                with solver._lock:
                    got = ctx.posterior_var(el, al, H=Hs, F=F, chi2_factor=chi2_factor, want_diag=want_diag, timing=t)
            else:
                got = ctx.posterior_var(el, al, H=Hs, F=F, chi2_factor=chi2_factor, want_diag=want_diag, timing=t)
            ms += t.get('ms', 0.0)
        finally:
            if own:
                ctx.close()
        pos = 0
        for e in mine:
            k = len(alpha_rows[e])
            out_var[e], out_prior[e] = got['var'][pos:pos + k], got['prior'][pos:pos + k]
            out_diag[e] = got['diag'][pos:pos + k] if want_diag else None
            pos += k
    if timing is not None:
        timing['ms'] = ms
        timing['reused_contexts'] = reused
    return out_var, out_prior, out_diag


# ---- one job: several elements of one kernel ------------------------------------------------------------------------

def element_errors(K, omega, items, alpha=None, windows=None, functionals=None, pointwise=False, default_name=None,
                   chi2_factor=1.0, device_ids=None, bryan=None, timing=None):
    """The error bars of the elements ``items`` of one kernel.  An item: dict(spec=..., H=(n_alpha, n_omega),
    alpha=(n_alpha,) scaled, analysis=analyzer results, probability=(n_alpha,) or None, B=preblur matrix or None).
    Returns a list of dicts, one per item (see ``TauMaxEnt.posterior_errors``)."""
    delta = np.asarray(omega.delta, dtype=float)
    n_omega = len(delta)
    n_win = 0 if windows is None else len(windows)
    Wrows = window_rows(omega, windows) if n_win else np.zeros((0, n_omega))
    Frows = functional_rows(functionals, n_omega) if functionals is not None else np.zeros((0, n_omega))
    n_fun = len(Frows)
    if n_win + n_fun == 0 and not pointwise:
        raise ValueError('nothing to compute: give windows=, functionals= or pointwise=True')
    B = items[0].get('B')
    # a window is the weight 1 on A delta inside it: the sum of H_i there, or with a preblur of (B H)_i delta_i
    rows = rows_on_H(np.concatenate([Wrows, Frows]), delta, B)
    blurred_points = pointwise and B is not None
    if blurred_points:
        rows = np.concatenate([rows, np.asarray(B, dtype=float)])      # A_i = (B H)_i: the rows of B as functionals
    want_diag = pointwise and B is None
    picks, hows = [], []
    for it in items:
        n_alpha = len(it['alpha'])
        idx, how = choose_alpha(alpha, n_alpha, it.get('analysis'), default_name)
        if how == 'bryan':
            logp = it.get('probability')
            if logp is None:
                raise ValueError('Probability not calculated. Cannot use BryanAnalyzer.')
            average = bool(bryan.average_by_integration) if bryan is not None else False
            good, p = bryan_weights(logp, it['alpha'], average)
            idx = list(np.nonzero(good)[0])
            it = dict(it, _p=p)
        picks.append(idx)
        hows.append((how, it.get('_p')))
    H_rows = [np.asarray(it['H'], dtype=float)[idx] for it, idx in zip(items, picks)]
    al_rows = [np.asarray(it['alpha'], dtype=float)[idx] for it, idx in zip(items, picks)]
    # rows that are not finite get NaN from the device; they are reported per element
    var, prior, diag = device_variances(K, [it['spec'] for it in items], H_rows, al_rows, rows if len(rows) else None,
                                        want_diag, chi2_factor=chi2_factor, device_ids=device_ids, timing=timing)
    outs = []
    for n, it in enumerate(items):
        Hn, an = H_rows[n], al_rows[n]
        how, p = hows[n]
        nf = len(rows)
        v = var[n] if nf else np.zeros((len(an), 0))
        pr = prior[n] if nf else np.zeros((len(an), 0))
        val = np.dot(Hn, rows.T) if nf else np.zeros((len(an), 0))
        if pointwise:
            if blurred_points:
                A_val, A_var, A_prior = val[:, n_win + n_fun:], v[:, n_win + n_fun:], pr[:, n_win + n_fun:]
            else:
                w = entropy_weights(Hn, it['spec']['D'], it['spec']['kind'])
                A_val = Hn / delta
                A_var = diag[n] / delta ** 2
                A_prior = w / (an[:, np.newaxis] * delta ** 2)
        bad = np.nonzero(~np.all(np.isfinite(Hn), axis=-1) |
                         (np.any(np.isnan(v), axis=-1) if nf else False) |
                         (np.any(np.isnan(diag[n]), axis=-1) if want_diag else False))[0]
        out = dict(alpha_index=np.array(picks[n]), alpha=an,
                   info=dict(nan_rows=[int(picks[n][b]) for b in bad]))
        if how == 'bryan':
            mean, mv = bryan_mixture(p, val, v)
            _, mp = bryan_mixture(p, val, pr)
            if pointwise:
                A_val, A_var = bryan_mixture(p, A_val, A_var)
                A_prior = bryan_mixture(p, np.zeros_like(A_prior), A_prior)[1]
            val, v, pr = mean, mv, mp
            out['weights'] = p
        elif how == 'one':
            val, v, pr = val[0], v[0], pr[0]
            out['alpha_index'], out['alpha'] = out['alpha_index'][0], out['alpha'][0]
            if pointwise:
                A_val, A_var, A_prior = A_val[0], A_var[0], A_prior[0]
        err, perr = np.sqrt(v), np.sqrt(pr)
        out['prior_err'] = perr[..., :n_win + n_fun]
        if n_win:
            out['window_weight'], out['window_err'] = val[..., :n_win], err[..., :n_win]
            out['window_prior_err'] = perr[..., :n_win]
        if n_fun:
            out['functional_value'], out['functional_err'] = val[..., n_win:n_win + n_fun], err[..., n_win:n_win + n_fun]
            out['functional_prior_err'] = perr[..., n_win:n_win + n_fun]
        if pointwise:
            out['A'], out['A_err'], out['A_prior_err'] = A_val, np.sqrt(A_var), np.sqrt(A_prior)
        outs.append(out)
    return outs


def find_bryan(analyzers):
    for a in analyzers or ():
        if isinstance(a, BryanAnalyzer):
            return a
    return None


def check_alpha(spec, result_alpha):
    a, b = np.asarray(spec['alpha'], dtype=float), np.asarray(result_alpha, dtype=float)
    if a.shape != b.shape or not np.allclose(a, b, rtol=1e-12, atol=0.0):
        raise ValueError('the alphas of the result are not those of this object (alpha_mesh and scale_alpha as they were '
                         'when the result was made are needed)')
