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

``posterior_samples`` draws spectra from the same Gaussian (``mxe_posterior_sample``) for error bars of what is not linear
in A.  The standard normals behind a draw come from a counter-based generator (Philox4x32-10 + Box-Muller) that
:func:`philox4x32_10` and :func:`sample_normals` mirror on the host, so a draw can be reproduced off the device.
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


# ---- the generator of mxe_normals / mxe_posterior_sample, mirrored in numpy ----------------------------------------

_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011, the Random123 constants): ``counter`` (..., 4) and ``key`` (..., 2) 32-bit words
    (broadcast against each other) -> (..., 4) uint32"""
    c = np.asarray(counter, dtype=np.uint64) & _M32
    k = np.asarray(key, dtype=np.uint64) & _M32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    for r in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2                    # (32 x 32 -> 64 bits: no overflow)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & _M32, (k1 + np.uint64(_PHILOX_W1)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def sample_normals(seed, stream, n_samples, n):
    """the standard normals (n_samples, n) that ``mxe_normals`` gives for ``(seed, stream)``: key (seed low, seed high),
    counter (j, s, stream low, stream high) for the pair j of sample s; u = (((x0 2^32 + x1) >> 11) + 0.5) 2^-53 from each
    half of the output, z_2j = sqrt(-2 ln u1) cos(2 pi u2), z_2j+1 = sqrt(-2 ln u1) sin(2 pi u2).  Row s depends on
    (seed, stream, s) alone."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    n_samples, n = int(n_samples), int(n)
    if n_samples < 1 or n < 1:
        raise ValueError('sample_normals: n_samples and n must be at least 1')
    npair = (n + 1) // 2
    ctr = np.empty((n_samples, npair, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(npair, dtype=np.uint64)[np.newaxis, :]
    ctr[..., 1] = np.arange(n_samples, dtype=np.uint64)[:, np.newaxis]
    ctr[..., 2], ctr[..., 3] = stream & 0xFFFFFFFF, stream >> 32
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    u1 = ((((x[..., 0] << np.uint64(32)) | x[..., 1]) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((((x[..., 2] << np.uint64(32)) | x[..., 3]) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    r, t = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    z = np.empty((n_samples, 2 * npair))
    z[:, 0::2], z[:, 1::2] = r * np.cos(t), r * np.sin(t)
    return np.ascontiguousarray(z[:, :n])


def stream_id(flat_element, complex_index, n_alpha, alpha_index):
    """the 64-bit stream of one (element, alpha): an element draws the same spectra alone and inside a matrix"""
    return (int(flat_element) * 2 + int(complex_index)) * int(n_alpha) + int(alpha_index)


def bryan_allotment(p, n_samples, seed, stream_base=0):
    """for every sample the index (into ``p``) of its alpha, drawn with the Bryan weights ``p`` from
    ``np.random.Generator(np.random.Philox(seed))`` (counter word 3 = ``stream_base``: elements draw independently)"""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError('n_samples must be at least 1')
    p = np.asarray(p, dtype=float)
    rng = np.random.Generator(np.random.Philox(key=int(seed) & (2 ** 64 - 1), counter=[0, 0, 0, int(stream_base)]))
    return rng.choice(len(p), size=n_samples, p=p / p.sum())


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


def _holds_data(solver, ctx, specs):
    """whether the staged context ``ctx`` of ``solver`` holds the data vectors of ``specs`` (``staged_context_for`` compares
    everything but them: the posterior does not depend on G)"""
    old = solver.__dict__.get('_staged', {}).get(id(ctx))
    G = None if old is None else old.get('G')
    return G is not None and len(G) == len(specs) and \
        all(np.shape(s['G']) == G[i].shape and np.array_equal(G[i], s['G']) for i, s in enumerate(specs))


def _per_device(K, specs, H_rows, alpha_rows, call, device_ids=None, timing=None, match_data=False):
    """One ``call(ctx, el, al, Hs, mine, t)`` per device for the elements ``specs`` of the kernel ``K``: element e (with
    the hidden images ``H_rows[e]`` (n_e, n_omega) at ``alpha_rows[e]`` (n_e)) goes to device e mod N, as the solve shards
    them; the devices are visited one after the other.  ``ctx``: the solver's staged context when there is one (the call
    then runs under the solver's lock), else one of its own.  ``el``, ``al``, ``Hs``: the problems of the elements
    ``mine``, concatenated; ``t``: the call's timing dict.  ``call`` returns a tuple of arrays with one row per problem
    (or None); per element the tuple of its rows is returned.  ``match_data``: a staged context is taken only when it
    holds the data vectors of ``specs`` too (what ``call`` computes depends on G)."""
    from .batch_solver import BatchSolver
    device_ids = tuple(device_ids) if device_ids else (0,)
    n = len(specs)
    out = [None] * n
    ms, reused = 0.0, 0
    for r, dev in enumerate(device_ids):
        mine = list(range(r, n, len(device_ids)))
        if not mine:
            continue
        sub = [specs[e] for e in mine]
        ctx, solver = BatchSolver.staged_context_for(K, sub, dev) if len(device_ids) == 1 else (None, None)
        if ctx is not None and match_data and not _holds_data(solver, ctx, sub):
            ctx = solver = None
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
                    got = call(ctx, el, al, Hs, mine, t)
            else:
                got = call(ctx, el, al, Hs, mine, t)
            ms += t.get('ms', 0.0)
        finally:
            if own:
                ctx.close()
        pos = 0
        for e in mine:
            k = len(alpha_rows[e])
            out[e] = tuple(None if a is None else a[pos:pos + k] for a in got)
            pos += k
    if timing is not None:
        timing['ms'] = ms
        timing['reused_contexts'] = reused
    return out


def device_variances(K, specs, H_rows, alpha_rows, F, want_diag, chi2_factor=1.0, device_ids=None, timing=None):
    """``mxe_posterior_var`` for the elements ``specs`` of the kernel ``K`` (see :func:`_per_device`): ONE call per device
    for everything.  Returns per element ``var``, ``prior`` (n_e, n_f) and ``diag`` (n_e, n_omega) or None."""
    def call(ctx, el, al, Hs, mine, t):
        got = ctx.posterior_var(el, al, H=Hs, F=F, chi2_factor=chi2_factor, want_diag=want_diag, timing=t)
        return got['var'], got['prior'], got.get('diag')
    got = _per_device(K, specs, H_rows, alpha_rows, call, device_ids, timing)
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got]


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


# ---- samples ---------------------------------------------------------------------------------------------------------

TRANSFORMS = ('linear', 'log')


def device_samples(K, specs, H_rows, alpha_rows, stream_rows, n_samples, seed, z_rows=None, chi2_factor=1.0, device_ids=None,
                   timing=None):
    """``mxe_posterior_sample`` for the elements ``specs`` of the kernel ``K`` (as :func:`device_variances`).  Returns per
    element ``delta`` (n_e, n_samples, n_omega)."""
    def call(ctx, el, al, Hs, mine, t):
        st = np.concatenate([np.asarray(stream_rows[e], dtype=np.uint64) for e in mine])
        zz = None if z_rows is None else np.concatenate([np.asarray(z_rows[e], dtype=float) for e in mine])
        return (ctx.posterior_sample(el, al, H=Hs, chi2_factor=chi2_factor, n_samples=n_samples, seed=seed, stream=st, z=zz,
                                     timing=t),)
    return [g[0] for g in _per_device(K, specs, H_rows, alpha_rows, call, device_ids, timing)]


def apply_transform(H, delta, transform):
    """a sample of H from the minimiser ``H`` (..., n_omega) and the Gaussian draw ``delta`` (..., n_samples, n_omega):
    ``'linear'`` H + delta; ``'log'`` H exp(delta / H), positive and equal to first order (normal entropy)"""
    H = np.asarray(H, dtype=float)[..., np.newaxis, :]
    if transform == 'linear':
        return H + delta
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return np.where(H > 0, H * np.exp(delta / np.where(H > 0, H, 1.0)), H + delta)


def element_samples(K, omega, items, n_samples=100, seed=0, alpha=None, transform='linear', z=None, default_name=None,
                    chi2_factor=1.0, device_ids=None, bryan=None, timing=None):
    """Draws from the Gaussian posterior of the elements ``items`` of one kernel.  An item: as in :func:`element_errors`,
    with ``stream`` = (flat element index) * 2 + complex index.  Returns a list of dicts, one per item (see
    ``TauMaxEnt.posterior_samples``)."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError('n_samples must be at least 1, got {}'.format(n_samples))
    if transform not in TRANSFORMS:
        raise ValueError('transform={!r}: one of {} is needed'.format(transform, TRANSFORMS))
    if transform == 'log' and any(it['spec']['kind'] != device.ENTROPY_NORMAL for it in items):
        raise ValueError("transform='log' needs the normal entropy (a positive H); plus-minus elements take 'linear'")
    delta = np.asarray(omega.delta, dtype=float)
    n_omega, nz = len(delta), len(delta) + len(np.array(K.S))
    B = items[0].get('B')
    picks, hows, allot = [], [], []
    for it in items:
        n_alpha = len(it['alpha'])
        idx, how = choose_alpha(alpha, n_alpha, it.get('analysis'), default_name)
        p = who = None
        if how == 'bryan':
            logp = it.get('probability')
            if logp is None:
                raise ValueError('Probability not calculated. Cannot use BryanAnalyzer.')
            average = bool(bryan.average_by_integration) if bryan is not None else False
            good, p = bryan_weights(logp, it['alpha'], average)
            who = np.nonzero(good)[0][bryan_allotment(p, n_samples, seed, it.get('stream', 0))]
            idx = sorted(set(int(i) for i in who))               # (only the alphas that own a sample are drawn from)
        picks.append(idx)
        hows.append((how, p))
        allot.append(who)
    z_rows = None
    if z is not None:
        if any(h == 'bryan' for h, _ in hows):
            raise ValueError("z= cannot be combined with alpha='bryan' (the allotment decides which normals are used)")
        z = np.asarray(z, dtype=float)
        z_rows = []
        for idx in picks:
            if z.shape not in ((n_samples, nz), (len(idx), n_samples, nz)):
                raise ValueError('z: the shape (n_samples, n_omega + n_s) = {} or ({}, n_samples, n_omega + n_s) is needed, '
                                 'got {}'.format((n_samples, nz), len(idx), z.shape))
            z_rows.append(np.broadcast_to(z, (len(idx), n_samples, nz)))
        if not np.all(np.isfinite(z)):
            raise ValueError('z holds values that are not finite')
    H_rows = [np.asarray(it['H'], dtype=float)[idx] for it, idx in zip(items, picks)]
    al_rows = [np.asarray(it['alpha'], dtype=float)[idx] for it, idx in zip(items, picks)]
    st_rows = [[it.get('stream', 0) * len(it['alpha']) + i for i in idx] for it, idx in zip(items, picks)]
    # with 'bryan' sample s takes the draw s of its alpha's stream: n_samples draws of every alpha that owns one
    deltas = device_samples(K, [it['spec'] for it in items], H_rows, al_rows, st_rows, n_samples, seed, z_rows=z_rows,
                            chi2_factor=chi2_factor, device_ids=device_ids, timing=timing)
    outs = []
    for n, it in enumerate(items):
        Hn, an, dn = H_rows[n], al_rows[n], deltas[n]
        how, p = hows[n]
        bad = np.nonzero(np.any(np.isnan(dn), axis=(1, 2)))[0]
        out = dict(alpha_index=np.array(picks[n]), alpha=an, seed=int(seed),
                   info=dict(nan_rows=[int(picks[n][b]) for b in bad]))
        Hs = apply_transform(Hn, dn, transform)                 # (n_e, n_samples, n_omega)
        if how == 'bryan':
            pos = np.searchsorted(np.array(picks[n]), allot[n])
            Hs = Hs[pos, np.arange(n_samples)]
            good = np.logical_not(np.isnan(np.asarray(it['probability'], dtype=float)))
            out['H'] = np.dot(p, np.asarray(it['H'], dtype=float)[good])
            out['alpha_index_samples'], out['weights'] = np.asarray(allot[n]), p
            out['alpha_index'], out['alpha'] = np.nonzero(good)[0], np.asarray(it['alpha'], dtype=float)[good]
        elif how == 'one':
            Hs, out['H'] = Hs[0], Hn[0]
            out['alpha_index'], out['alpha'] = out['alpha_index'][0], out['alpha'][0]
        else:
            out['H'] = Hn
        out['H_samples'] = Hs
        out['A_samples'] = Hs / delta if B is None else np.dot(Hs, np.asarray(B, dtype=float).T)
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
