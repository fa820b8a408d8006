"""The linear response of a MaxEnt continuation (``TauMaxEnt.resolution``, ``TauMaxEnt.default_model_response`` and their
element-wise counterparts): what the continuation does to a feature that is really there.

Differentiating the stationarity condition of ``Q = eta chi2 / 2 - alpha~ S`` at the minimiser gives, exactly,

    (eta K^T Sigma^-1 K + alpha~ diag(1/w)) dH = eta K^T Sigma^-1 dG + alpha~ diag(1/w) (H o dlnD)

with ``w = H`` (normal entropy) or ``sqrt(H^2 + 4 D^2)`` (plus-minus entropy; dS/dH = -asinh(H / 2D), whose derivative with
respect to ln D at fixed H is +H/w).  With the posterior covariance Gamma of :mod:`maxent_amd.posterior`:

    dH = Gamma eta K^T Sigma^-1 dG                           response to the data
    dH = R dH_t,   R = I - alpha~ Gamma diag(1/w)            response to the true spectrum (dG = K dH_t, H = A delta_omega)
    dH = (I - R)(H o dlnD)                                   response to the default model, both entropies

``R = diag(w) S`` with a symmetric ``S``: column j of R is the point-spread function of a unit of weight at omega_j, row j
the Backus-Gilbert averaging kernel of the value returned there, ``R_jj`` in [0, 1] the share of point j that the data
decide (``1 - var / prior`` of ``posterior_errors(pointwise=True)``), ``tr R`` the number of good data of
``fit_diagnostics``.  With a preblur (A = B H) a perturbation of the true spectrum reaches H only through the data,
``dG = K_delta dA_t``, and ``dA = B dH``.

``mxe_response`` applies these maps on the device (one call per device and block of right-hand sides for all matrix
elements and alphas); this module is the host glue: the right-hand sides, the summaries of a point-spread function, the
shape of what is returned.  There is no CPU path: without the library and a GPU
:class:`maxent_amd.device.MaxEntDeviceError` is raised.
"""

import numpy as np

from . import posterior

#: values of the largest array of one ``mxe_response`` call made by the drivers (the mesh points go in chunks)
CHUNK_VALUES = 1 << 24


# ---- right-hand sides (no device) ------------------------------------------------------------------------------------

def snap_points(omega, omega0=None):
    """mesh indices of the points ``omega0`` (each snapped to the nearest mesh point; None: every mesh point)"""
    w = np.asarray(omega, dtype=float)
    if omega0 is None:
        return np.arange(len(w))
    x = np.atleast_1d(np.asarray(omega0, dtype=float))
    if x.ndim != 1 or x.size == 0 or not np.all(np.isfinite(x)):
        raise ValueError('omega0: a finite value or a sequence of finite values is needed, got {!r}'.format(omega0))
    if x.min() < w.min() or x.max() > w.max():
        raise ValueError('omega0: {} .. {} reaches outside the omega mesh [{}, {}]'.format(x.min(), x.max(), w.min(), w.max()))
    return np.argmin(np.abs(w[np.newaxis, :] - x[:, np.newaxis]), axis=1)


def unit_rows(index, n_omega):
    """unit weights at the mesh indices ``index``: rows e_j of the identity"""
    index = np.asarray(index, dtype=int)
    rows = np.zeros((len(index), n_omega))
    rows[np.arange(len(index)), index] = 1.0
    return rows


def spectrum_rows(test, delta):
    """test spectra ``dA_t`` (n_test, n_omega) as perturbations of the hidden image: ``dA_t o delta_omega``"""
    delta = np.asarray(delta, dtype=float)
    t = np.atleast_2d(np.asarray(test, dtype=float))
    if t.ndim != 2 or t.shape[1] != len(delta):
        raise ValueError('test: shape (n_test, n_omega = {}) is needed, got {}'.format(len(delta), np.shape(test)))
    if not np.all(np.isfinite(t)):
        raise ValueError('test holds values that are not finite')
    return t * delta[np.newaxis, :]


def default_model_rows(H, dlogD):
    """``H o dlnD``: (n_alpha, n_dir, n_omega) from H (n_alpha, n_omega) and the directions ``dlogD`` (n_dir, n_omega)"""
    H = np.atleast_2d(np.asarray(H, dtype=float))
    d = check_dlogD(dlogD, H.shape[-1])
    return H[:, np.newaxis, :] * d[np.newaxis, :, :]


def check_dlogD(dlogD, n_omega):
    d = np.asarray(dlogD, dtype=float)
    if d.ndim != 2 or d.shape[1] != n_omega or d.shape[0] < 1:
        raise ValueError('dlogD: shape (n_dir, n_omega = {}) is needed, got {}'.format(n_omega, np.shape(dlogD)))
    if not np.all(np.isfinite(d)):
        raise ValueError('dlogD holds values that are not finite')
    return d


def data_rows(K_delta, dA, T=None, err=1.0):
    """perturbations ``dA`` (n, n_omega) of the true spectrum as whitened perturbations of the data, in the rows of a data
    set: ``dG = K_delta dA``, rotated by the set's ``T`` (the rows of ``T`` are the eigenvectors of its covariance, as
    ``_set_eigenbasis`` applies them) and divided by its errors (one per row, as ``set_error`` holds them).
    Returns (n, rows)."""
    dG = np.dot(np.asarray(K_delta), np.atleast_2d(np.asarray(dA, dtype=float)).T)
    if T is not None:
        dG = np.dot(np.asarray(T), dG)
    if np.iscomplexobj(dG):
        if np.max(np.abs(dG.imag)) > 1e-12 * max(np.max(np.abs(dG.real)), 1e-300):
            raise ValueError('the rotated data perturbation is complex: stack real and imaginary parts first')
        dG = dG.real
    err = np.asarray(err, dtype=float) * np.ones(dG.shape[0])
    return np.ascontiguousarray((dG / err[:, np.newaxis]).T)


# ---- summaries of a point-spread function (no device) ----------------------------------------------------------------

def fwhm(omega, p):
    """full width at half maximum of the lobe of ``p`` (n_omega) that holds its maximum, with linear interpolation between
    mesh points; NaN when a side does not reach half the maximum on the mesh (or the maximum is not positive)"""
    w, p = np.asarray(omega, dtype=float), np.asarray(p, dtype=float)
    if not np.all(np.isfinite(p)):
        return np.nan
    m = int(np.argmax(p))
    half = 0.5 * p[m]
    if not half > 0.0:
        return np.nan
    i = m
    while i >= 0 and p[i] > half:
        i -= 1
    k = m
    while k < len(p) and p[k] > half:
        k += 1
    if i < 0 or k >= len(p):
        return np.nan
    left = w[i] + (half - p[i]) / (p[i + 1] - p[i]) * (w[i + 1] - w[i])
    right = w[k - 1] + (half - p[k - 1]) / (p[k] - p[k - 1]) * (w[k] - w[k - 1])
    return float(right - left)


def psf_summaries(omega, delta, psf, omega0):
    """Summaries of point-spread functions ``psf`` (..., n_pts, n_omega; p_i = dA(omega_i) for a unit of weight at
    ``omega0`` (n_pts)): ``weight`` = sum p_i delta_i, ``centroid`` = sum omega_i p_i delta_i / weight, ``shift`` =
    centroid - omega0, ``spread`` = sqrt(sum (omega_i - omega0)^2 p_i^2 delta_i / sum p_i^2 delta_i) (Backus-Gilbert's form:
    defined with negative side lobes too), ``peak`` (the position of the maximum), ``height`` (its value) and ``fwhm``
    (:func:`fwhm`).  Each (..., n_pts)."""
    w, d = np.asarray(omega, dtype=float), np.asarray(delta, dtype=float)
    p = np.asarray(psf, dtype=float)
    x0 = np.asarray(omega0, dtype=float)
    weight = np.sum(p * d, axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        centroid = np.sum(p * (w * d), axis=-1) / weight
        dist2 = (w[np.newaxis, :] - x0[:, np.newaxis]) ** 2
        spread = np.sqrt(np.sum(dist2 * p * p * d, axis=-1) / np.sum(p * p * d, axis=-1))
    bad = np.any(np.isnan(p), axis=-1)
    top = np.argmax(np.where(np.isnan(p), -np.inf, p), axis=-1)
    flat = p.reshape(-1, p.shape[-1])
    width = np.array([fwhm(w, row) for row in flat]).reshape(p.shape[:-1])
    return dict(weight=weight, centroid=centroid, shift=centroid - x0, spread=spread,
                peak=np.where(bad, np.nan, w[top]), height=np.where(bad, np.nan, np.take_along_axis(p, top[..., np.newaxis], -1)[..., 0]),
                fwhm=width)


def choose_alpha(alpha, n_alpha, analysis, default_name):
    """``alpha=`` of resolution / default_model_response: as :func:`maxent_amd.posterior.choose_alpha` without ``'bryan'``
    (the mixture weights depend on the data, so the mixture is not a linear map)"""
    if isinstance(alpha, str) and alpha == 'bryan':
        raise ValueError("alpha='bryan': the Bryan weights depend on the data, so the mixture has no linear response; "
                         "use 'all', an analyzer name or indices")
    return posterior.choose_alpha(alpha, n_alpha, analysis, default_name)


# ---- the device part -------------------------------------------------------------------------------------------------

def device_response(K, specs, H_rows, alpha_rows, requests, chi2_factor=1.0, device_ids=None, timing=None):
    """``mxe_response`` for the elements ``specs`` of the kernel ``K`` (see :func:`maxent_amd.posterior._per_device`; a
    staged context of the solver is taken whatever data it holds: the response does not depend on G).  ``requests``: a
    list of ``(space, weighted, F)`` with ``F`` a list of per-element right-hand sides, (n_rhs, ld_e) for all alphas of
    the element alike or (n_e, n_rhs, ld_e); the rows of data-space sides are padded to the longest element.  Returns per
    request the list of per-element X (n_e, n_rhs, n_omega)."""
    launches = [0]

    def call(ctx, el, al, Hs, mine, t):
        got, ms = [], 0.0
        for space, weighted, F in requests:
            ld = max(np.shape(F[e])[-1] for e in mine)
            parts = []
            for e in mine:
                Fe = np.asarray(F[e], dtype=float)
                if Fe.ndim == 2:
                    Fe = np.broadcast_to(Fe, (len(alpha_rows[e]),) + Fe.shape)
                parts.append(np.pad(Fe, [(0, 0), (0, 0), (0, ld - Fe.shape[-1])]))
            tt = {}
            got.append(ctx.response(el, al, np.concatenate(parts), H=Hs, chi2_factor=chi2_factor, space=space,
                                    weighted=weighted, timing=tt))
            ms += tt.get('ms', 0.0)
            launches[0] += tt.get('launches', 0)
        t['ms'] = ms
        return tuple(got)
    got = posterior._per_device(K, specs, H_rows, alpha_rows, call, device_ids, timing, match_data=False)
    if timing is not None:
        timing['launches'] = launches[0]
    return [[g[r] for g in got] for r in range(len(requests))]


def _pick(items, alpha, default_name):
    picks, hows = [], []
    for it in items:
        idx, how = choose_alpha(alpha, len(it['alpha']), it.get('analysis'), default_name)
        picks.append(idx)
        hows.append(how)
    H_rows = [np.asarray(it['H'], dtype=float)[idx] for it, idx in zip(items, picks)]
    al_rows = [np.asarray(it['alpha'], dtype=float)[idx] for it, idx in zip(items, picks)]
    return picks, hows, H_rows, al_rows


def element_resolution(K, omega, items, omega0=None, alpha=None, test=None, default_name=None, chi2_factor=1.0,
                       device_ids=None, timing=None, note=None):
    """The resolution of the elements ``items`` of one kernel.  An item: dict(spec=..., H=(n_alpha, n_omega),
    alpha=(n_alpha,) scaled, analysis=analyzer results, B=preblur matrix or None).  Returns a list of dicts, one per item
    (see ``TauMaxEnt.resolution``).  ``note``: called with a message when something is left out (the preblur case)."""
    w_mesh = np.asarray(omega, dtype=float)
    delta = np.asarray(omega.delta, dtype=float)
    n_omega = len(delta)
    index = snap_points(w_mesh, omega0)
    x0 = w_mesh[index]
    trows = None if test is None else spectrum_rows(test, delta)
    picks, hows, H_rows, al_rows = _pick(items, alpha, default_name)
    specs = [it['spec'] for it in items]
    B = items[0].get('B')
    blurred = B is not None
    if blurred:
        B = np.asarray(B, dtype=float)
        if note is not None:
            note('resolution with a PreblurKernel: psf, image and summaries refer to A = B H and go through the data; '
                 'averaging_kernel is not computed (None).')
        K_delta = np.asarray(K.K_delta)
    P = sum(len(a) for a in al_rows)
    ld_max = n_omega if not blurred else max(n_omega, max(len(s['G']) for s in specs))
    chunk = max(1, min(len(index), CHUNK_VALUES // max(1, P * ld_max)))
    # every chunk of mesh points is a request (two without a preblur: R and S) of ONE visit of the device: the elements are
    # staged once, whatever the number of chunks
    starts = list(range(0, len(index), chunk))
    requests = []
    for c0 in starts:
        units = unit_rows(index[c0:c0 + chunk], n_omega)
        if blurred:
            # a unit of weight at omega_j: dA_t o delta = e_j, so dA_t = e_j / delta_j
            requests.append(('data', True, [data_rows(K_delta, units / delta[np.newaxis, :], s.get('T'), s['err']) for s in specs]))
        else:
            requests += [('model', True, [units] * len(specs)), ('model', False, [units] * len(specs))]
    if trows is not None:
        requests.append(('data', True, [data_rows(K_delta, trows / delta[np.newaxis, :], s.get('T'), s['err']) for s in specs])
                        if blurred else ('model', True, [trows] * len(specs)))
    got = device_response(K, specs, H_rows, al_rows, requests, chi2_factor=chi2_factor, device_ids=device_ids, timing=timing)
    per = 1 if blurred else 2
    psf = [np.empty((len(a), len(index), n_omega)) for a in al_rows]
    avk = None if blurred else [np.empty((len(a), len(index), n_omega)) for a in al_rows]
    for n, it in enumerate(items):
        w = None if blurred else posterior.entropy_weights(H_rows[n], it['spec']['D'], it['spec']['kind'])
        for c, c0 in enumerate(starts):
            sel = index[c0:c0 + chunk]
            if blurred:
                psf[n][:, c0:c0 + chunk] = np.dot(got[c][n], B.T)
            else:
                psf[n][:, c0:c0 + chunk] = got[per * c][n] / delta
                # row j of R = diag(w) S from column j of the symmetric S: r_j(omega_i) = w_j S_ji / delta_j
                avk[n][:, c0:c0 + chunk] = got[per * c + 1][n] * (w[:, sel] / delta[sel])[:, :, np.newaxis]
    image = None if trows is None else [np.dot(g, B.T) if blurred else g / delta for g in got[-1]]
    outs = []
    for n, it in enumerate(items):
        p = psf[n]
        out = dict(index=index, omega0=x0, alpha_index=np.array(picks[n]), alpha=al_rows[n], psf=p,
                   averaging_kernel=None if blurred else avk[n])
        out.update(psf_summaries(w_mesh, delta, p, x0))
        # the share of point j that the data decide: R_jj (with a preblur: of the unit of weight what returns at its own point)
        out['data_share'] = p[:, np.arange(len(index)), index] * delta[index]
        if image is not None:
            out['image'] = image[n]
        bad = np.nonzero(np.any(np.isnan(p), axis=(1, 2)))[0]
        out['info'] = dict(nan_rows=[int(picks[n][b]) for b in bad])
        if hows[n] == 'one':
            for name in out:
                if name not in ('index', 'omega0', 'info') and out[name] is not None:
                    out[name] = out[name][0]
        outs.append(out)
    return outs


def element_default_model_response(K, omega, items, dlogD, alpha=None, default_name=None, chi2_factor=1.0, device_ids=None,
                                   timing=None):
    """The response of the elements ``items`` of one kernel to a change ``dlogD`` (n_dir, n_omega) of the logarithm of
    their default models: ``dH = (I - R)(H o dlnD)``, ``dA = dH / delta_omega`` (``B dH`` with a preblur).  Items as in
    :func:`element_resolution`.  Returns a list of dicts, one per item (see ``TauMaxEnt.default_model_response``)."""
    delta = np.asarray(omega.delta, dtype=float)
    d = check_dlogD(dlogD, len(delta))
    picks, hows, H_rows, al_rows = _pick(items, alpha, default_name)
    F = [default_model_rows(H, d) for H in H_rows]
    got = device_response(K, [it['spec'] for it in items], H_rows, al_rows, [('model', True, F)], chi2_factor=chi2_factor,
                          device_ids=device_ids, timing=timing)[0]
    outs = []
    for n, it in enumerate(items):
        dH = F[n] - got[n]
        B = it.get('B')
        dA = dH / delta if B is None else np.dot(dH, np.asarray(B, dtype=float).T)
        bad = np.nonzero(np.any(np.isnan(dA), axis=(1, 2)))[0]
        out = dict(alpha_index=np.array(picks[n]), alpha=al_rows[n], dH=dH, dA=dA,
                   info=dict(nan_rows=[int(picks[n][b]) for b in bad]))
        if hows[n] == 'one':
            for name in ('alpha_index', 'alpha', 'dH', 'dA'):
                out[name] = out[name][0]
        outs.append(out)
    return outs
