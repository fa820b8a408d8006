"""Diagnostics of a MaxEnt fit (``TauMaxEnt.fit_diagnostics``, ``ElementwiseMaxEnt.fit_diagnostics``).

They all come from the hat matrix of the fit, the derivative of the fitted whitened data ``Sigma^-1/2 K H`` with respect
to the whitened data ``Sigma^-1/2 G``.  Differentiating the stationarity condition of ``Q = eta chi2 / 2 - alpha~ S`` gives

    (eta K^T Sigma^-1 K + alpha~ diag(1/w)) dH = eta K^T Sigma^-1 dG,      w = H  |  sqrt(H^2 + 4 D^2)  (plus-minus entropy)

so that at the minimiser, exactly, with ``a = alpha~ / eta``

    Hat = Sigma^-1/2 K (K^T Sigma^-1 K + a diag(1/w))^-1 K^T Sigma^-1/2
    h_i = Hat_ii                      the leverage of data point i: how much of its own fitted value it decides
    N_g = tr Hat                      the number of good data (Gull; Jarrell & Gubernatis 1996, section 4)
    r   = Sigma^-1/2 (K H - G)        the normalised residuals, sum_i r_i^2 = chi2

``mxe_fit_diagnostics`` computes h, N_g, r and chi2 (one call per device for all matrix elements and alphas); this
module is the host glue and the small formulas on top: studentized residuals, the lag-one autocorrelation of the
residuals, generalised cross-validation and the classic criterion ``-2 a S = N_g`` as rules for alpha.  There is no CPU
path: without the library and a GPU :class:`maxent_amd.device.MaxEntDeviceError` is raised.

A linearised leave-one-out score ``sum (r_i / (1 - h_i))^2`` is not offered: the end points of G(tau) have leverages
of 1 - O(1e-6) on small problems and make it meaningless.
"""

import numpy as np

from . import posterior


# ---- host formulas (no device) ---------------------------------------------------------------------------------------

def studentized(residual, leverage):
    """``r / sqrt(1 - h)``; NaN where ``1 - h < 1e-12`` (a point that the fit reproduces by construction)"""
    r, h = np.asarray(residual, dtype=float), np.asarray(leverage, dtype=float)
    one = 1.0 - h
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(one >= 1e-12, r / np.sqrt(np.where(one >= 1e-12, one, 1.0)), np.nan)


def autocorr(residual):
    """lag-one autocorrelation ``sum_i r_i r_{i+1} / sum_i r_i^2`` along the last axis; NaN entries (padding) are left
    out of both sums, a row without a finite pair gives NaN"""
    r = np.asarray(residual, dtype=float)
    if r.shape[-1] < 2:
        return np.full(r.shape[:-1], np.nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        num = np.nansum(r[..., :-1] * r[..., 1:], axis=-1)
        den = np.nansum(r * r, axis=-1)
        pairs = np.sum(np.isfinite(r[..., :-1] * r[..., 1:]), axis=-1)
        return np.where((pairs > 0) & (den > 0), num / np.where(den > 0, den, 1.0), np.nan)


def gcv(chi2, n_good, n_rows):
    """generalised cross-validation score ``n chi2 / (n - N_g)^2`` (Golub, Heath & Wahba 1979 with the hat matrix of
    the fit): it does not trust the absolute size of the error bars.  NaN where ``n - N_g`` is not positive."""
    chi2, n_good = np.asarray(chi2, dtype=float), np.asarray(n_good, dtype=float)
    left = float(n_rows) - n_good
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(left > 0, float(n_rows) * chi2 / np.where(left > 0, left, 1.0) ** 2, np.nan)


def good_data_ratio(a, S, n_good):
    """``-2 a S / N_g`` with ``a = alpha~ / eta``: 1 at the alpha of classic MaxEnt"""
    a, S, n_good = np.asarray(a, dtype=float), np.asarray(S, dtype=float), np.asarray(n_good, dtype=float)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(n_good > 0, -2.0 * a * S / np.where(n_good > 0, n_good, 1.0), np.nan)


def index_gcv(score):
    """the alpha index of the smallest GCV score (NaN entries are left out; all NaN: ValueError)"""
    score = np.asarray(score, dtype=float)
    if np.all(np.isnan(score)):
        raise ValueError('no alpha has a GCV score')
    return int(np.nanargmin(score))


def index_classic(ratio):
    """the alpha index where ``-2 a S / N_g`` is closest to 1 on the logarithmic scale (entries that are NaN or not
    positive are left out; none left: ValueError)"""
    ratio = np.asarray(ratio, dtype=float)
    with np.errstate(divide='ignore', invalid='ignore'):
        dist = np.abs(np.log(np.where(ratio > 0, ratio, np.nan)))
    if np.all(np.isnan(dist)):
        raise ValueError('no alpha has a positive ratio -2 a S / N_g')
    return int(np.nanargmin(dist))


def choose_alpha(alpha, n_alpha, analysis, default_name):
    """``alpha=`` of fit_diagnostics: as :func:`maxent_amd.posterior.choose_alpha` without ``'bryan'`` (a mixture of
    diagnostics over alpha means nothing)"""
    if isinstance(alpha, str) and alpha == 'bryan':
        raise ValueError("alpha='bryan': fit diagnostics belong to one alpha each; use 'all', an analyzer name or indices")
    return posterior.choose_alpha(alpha, n_alpha, analysis, default_name)


# ---- the device part -------------------------------------------------------------------------------------------------

def device_diagnostics(K, specs, H_rows, alpha_rows, chi2_factor=1.0, device_ids=None, timing=None):
    """``mxe_fit_diagnostics`` for the elements ``specs`` of the kernel ``K`` (see :func:`maxent_amd.posterior._per_device`):
    ONE call per device for everything.  Returns per element ``n_good``, ``chi2`` (n_e), ``residual`` and ``leverage``
    (n_e, rows of the element)."""
    def call(ctx, el, al, Hs, mine, t):
        got = ctx.fit_diagnostics(el, al, H=Hs, chi2_factor=chi2_factor, timing=t)
        return got['n_good'], got['chi2'], got['residual'], got['leverage']
    got = posterior._per_device(K, specs, H_rows, alpha_rows, call, device_ids, timing, match_data=True)
    out = []
    for s, g in zip(specs, got):
        n = len(s['G'])
        out.append((g[0], g[1], g[2][:, :n], g[3][:, :n]))
    return out


def element_diagnostics(K, items, alpha='all', default_name=None, chi2_factor=1.0, device_ids=None, timing=None):
    """The diagnostics of the elements ``items`` of one kernel.  An item: dict(spec=..., H=(n_alpha, n_omega),
    alpha=(n_alpha,) scaled, S=(n_alpha,), A=(n_alpha, n_omega), analysis=analyzer results).  Returns a list of dicts, one
    per item (see ``TauMaxEnt.fit_diagnostics``)."""
    picks, hows = [], []
    for it in items:
        idx, how = choose_alpha(alpha, len(it['alpha']), it.get('analysis'), default_name)
        picks.append(idx)
        hows.append(how)
    H_rows = [np.asarray(it['H'], dtype=float)[idx] for it, idx in zip(items, picks)]
    al_rows = [np.asarray(it['alpha'], dtype=float)[idx] for it, idx in zip(items, picks)]
    got = device_diagnostics(K, [it['spec'] for it in items], H_rows, al_rows, chi2_factor=chi2_factor,
                             device_ids=device_ids, timing=timing)
    outs = []
    for n, it in enumerate(items):
        ng, chi2, r, h = got[n]
        an = al_rows[n]
        n_rows = r.shape[1]
        S = np.asarray(it['S'], dtype=float)[picks[n]]
        rotated = it['spec'].get('T') is not None
        bad = np.nonzero(np.isnan(ng) | np.isnan(chi2))[0]
        out = dict(alpha_index=np.array(picks[n]), alpha=an, n_good=ng, chi2=chi2, residual=r, leverage=h,
                   studentized=studentized(r, h),
                   autocorr=np.full(len(an), np.nan) if rotated else autocorr(r),
                   gcv=gcv(chi2, ng, n_rows),
                   good_data_ratio=good_data_ratio(an / chi2_factor, S, ng),
                   info=dict(nan_rows=[int(picks[n][b]) for b in bad]))
        if isinstance(alpha, str) and alpha == 'all':
            A = np.asarray(it['A'])
            for name, rule, key in (('gcv', index_gcv, 'gcv'), ('classic', index_classic, 'good_data_ratio')):
                try:
                    i = rule(out[key])
                except ValueError:
                    i = -1
                out['alpha_index_' + name] = i
                out['A_' + name] = np.array(A[i]) if i >= 0 else np.full(A.shape[1:], np.nan)
        elif hows[n] == 'one':
            for name in ('alpha_index', 'alpha', 'n_good', 'chi2', 'residual', 'leverage', 'studentized', 'autocorr', 'gcv',
                         'good_data_ratio'):
                out[name] = out[name][0]
        outs.append(out)
    return outs
