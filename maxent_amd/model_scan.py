"""Default-model scans (``TauMaxEnt.default_model_scan``, ``ElementwiseMaxEnt.default_model_scan``).  Not in the
reference, whose users loop ``run()`` over their default models, one object per model.

The default model is the one input of a continuation that is chosen by hand.  ``default_model_response`` says how much
of A(omega) comes from it in the linear regime; here the same data are continued under a whole family of models, and the
data say which they prefer: ``NormalLogProbability`` gives log p(alpha, D | G), its integral over alpha

    Z(D) = int d alpha~ p(alpha~, D | G)  ~  sum_k p_k |delta alpha~_k|

is the evidence of the model D (Bryan 1990; Jarrell & Gubernatis 1996, section 5.3), comparable between models on the
same data, error bars, omega mesh and alpha mesh.  With a prior P(D) the weights P(D) Z(D) / sum give the model-averaged
spectrum and the spread between the models.

All models of a matrix element are scans of ONE launch of the solver per device -- a spec carries its own ``D`` and
start vector --, ``mxe_logdet`` runs over the whole launch, and ``mxe_evidence_reduce`` reads the H rows where they lie:
no H row crosses to the host.  This module is the host glue: the specs, which scans form which group, the shape of what
is returned.  There is no CPU path.
"""

import numpy as np

from .analyzers import get_delta
from .default_models import BaseDefaultModel
from .posterior import window_rows, functional_rows, rows_on_H, find_bryan
from .probabilities import NormalLogProbability
from .resampling import SLOTS, BLUR_CHUNK, check_minimizer, choose_slot


# ---- host glue (no device) ------------------------------------------------------------------------------------------

def check_models(models, omega):
    """``models=`` of default_model_scan -> (names, list of D arrays): a list, or a dict name -> model, of
    ``BaseDefaultModel`` objects on the mesh ``omega`` or arrays of length n_omega holding ``D`` (density x delta)"""
    n_omega = len(omega)
    if isinstance(models, dict):
        names, entries = [str(k) for k in models.keys()], list(models.values())
    else:
        if isinstance(models, (BaseDefaultModel, np.ndarray)) and np.ndim(models) < 2:
            raise ValueError('models: a list or a dict of default models is needed')
        entries = list(models)
        names = [str(n) for n in range(len(entries))]
    if not entries:
        raise ValueError('models: at least one default model is needed')
    out = []
    for name, m in zip(names, entries):
        if isinstance(m, BaseDefaultModel):
            if len(m.omega) != n_omega or not np.array_equal(np.asarray(m.omega, dtype=float), np.asarray(omega, dtype=float)):
                raise ValueError('model {}: it is not on the omega mesh of this object'.format(name))
            D = np.array(m.D, dtype=float)
        else:
            D = np.array(m, dtype=float)
        if D.shape != (n_omega,):
            raise ValueError('model {}: D of shape {} where the omega mesh has {} points'.format(name, D.shape, n_omega))
        if not np.all(np.isfinite(D)) or not np.all(D > 0):
            raise ValueError('model {}: D must be finite and positive on every point of the mesh'.format(name))
        out.append(D)
    return names, out


def check_prior(prior, n_models):
    """``prior=`` of default_model_scan -> log P(model) (n_models), -inf for a model that is switched off; None: equal"""
    if prior is None:
        return None
    p = np.asarray(prior, dtype=float)
    if p.shape != (n_models,):
        raise ValueError('prior: one value per model ({}) is needed, got the shape {}'.format(n_models, p.shape))
    if not np.all(np.isfinite(p)) or np.any(p < 0):
        raise ValueError('prior: finite values that are not negative are needed')
    if not p.sum() > 0:
        raise ValueError('prior: it sums to 0')
    with np.errstate(divide='ignore'):
        return np.log(p / p.sum())


def log_measure(alpha):
    """log |get_delta(alpha~)|: the measure of the evidence integral on the alpha mesh (one alpha: 0)"""
    alpha = np.asarray(alpha, dtype=float)
    if len(alpha) < 2:
        return np.zeros(len(alpha))
    d = np.abs(get_delta(alpha))
    if not np.all(d > 0):
        raise ValueError('the alpha mesh holds the same value twice: it defines no measure for the evidence integral')
    return np.log(d)


def choose_rows(alpha, analyzers, n_alpha):
    """``alpha=`` of default_model_scan -> (row_mode of ``mxe_evidence_reduce``, slot of ``SLOTS`` or None, fixed index or
    None)"""
    if isinstance(alpha, str) and alpha.lower() == 'bryan':
        return 0, None, None
    if isinstance(alpha, str) and alpha.lower() == 'classic':
        return 1, None, None
    if alpha is None:
        raise ValueError("alpha: 'bryan', 'classic', one of {} or an index is needed".format(', '.join(SLOTS)))
    slot, fixed = choose_slot(alpha, analyzers, n_alpha)
    return 2, slot, fixed


# ---- the device part: the scans of all models of several elements of one kernel ---------------------------------------

def element_model_scan(K, omega, loop, templates, models, prior=None, alpha='bryan', windows=None, functionals=None,
                       pointwise=True, keep_models=True, device_ids=None):
    """The default-model scans of the elements ``templates`` (their specs, as ``MaxEntLoop.make_spec`` makes them) of one
    kernel.  ``models``: list of D arrays, ``prior``: log P(model) or None (:func:`check_models`, :func:`check_prior`).
    Element e is solved on device e mod N -- all its models on that device, one launch per device -- and reduced there.
    Returns (list of dicts, one per element, info)."""
    from .batch_solver import BatchSolver, directions_to_keep
    from .maxent_loop import solve_elements, select_params
    check_minimizer(loop)
    delta = np.asarray(omega.delta, dtype=float)
    n_omega = len(delta)
    n_elem, n_mod = len(templates), len(models)
    n_alpha = len(templates[0]['alpha'])
    n_win = 0 if windows is None else len(windows)
    Wrows = window_rows(omega, windows) if n_win else np.zeros((0, n_omega))
    Frows = functional_rows(functionals, n_omega) if functionals is not None else np.zeros((0, n_omega))
    n_fun = len(Frows)
    B = loop.A_of_H.matrix()
    rows = rows_on_H(np.concatenate([Wrows, Frows]), delta, B)          # weights on H (with a preblur: on A = B H)
    mode, slot, fixed = choose_rows(alpha, loop.analyzers, n_alpha)
    select = None
    if slot is not None:
        sel = select_params(loop.analyzers)
        deg, gamma = (sel[0], sel[1]) if sel is not None else (0, 0.2)
        select = (deg, gamma, slot, False)          # (the rows of the picks stay on the device)
    bryan = find_bryan(loop.analyzers)
    prob = loop.probability if loop.probability is not None else NormalLogProbability()
    log_prior = None if prior is None else np.asarray(prior, dtype=float)
    ids = tuple(device_ids) if device_ids else (loop.device_id,)
    N = len(ids)
    per_dev = [[e for e in range(n_elem) if e % N == r] for r in range(N)]
    outs = [None] * n_elem
    info = dict(kernel_ms=0.0, reduce_ms=0.0, launches=0, reduce_launches=0, devices=[])
    begun = []
    try:
        for r, dev in enumerate(ids):
            if not per_dev[r]:
                continue
            specs = [loop.spec_with_model(templates[e], D) for e in per_dev[r] for D in models]
            solver = BatchSolver.for_kernel(K, (dev,), keep=directions_to_keep(K, specs, None, chi2_factor=loop.cost_function.chi2_factor))
            solver._lock.acquire()              # (until this device's rows are reduced: nobody else launches on its contexts)
            begun.append([r, solver, specs, None])
            begun[-1][3] = solve_elements(K, specs, loop.minimizer, device_ids=(dev,),
                                          chi2_factor=loop.cost_function.chi2_factor, select=select, want_logdet=True,
                                          want_H=False, defer=True)
        for entry in begun:
            r, solver, specs, end = entry
            entry[3] = None
            sols, launch = end()
            if solver.last_info is not launch:
                raise RuntimeError('default_model_scan: the launch ran on another solver than the one that was locked')
            info['kernel_ms'] = max(info['kernel_ms'], launch.get('kernel_ms', 0.0))
            info['launches'] += 1
            info['devices'].append(ids[r])
            for k in ('audit_max', 'audit_problems'):
                if k in launch:
                    info[k] = max(info.get(k, 0.0), launch[k]) if k == 'audit_max' else info.get(k, 0) + launch[k]
            mine = per_dev[r]
            n_scan = len(mine) * n_mod
            logp = np.stack([np.asarray(prob.from_logdet(s['logdet'], s['alpha'], s['Q'], n_omega), dtype=float) for s in sols])
            log_quad = log_measure(specs[0]['alpha'])
            log_mix = log_quad if (bryan is not None and bryan.average_by_integration) else np.zeros(n_alpha)
            pick = None
            if mode == 2:
                pick = np.full(n_scan, fixed, dtype=np.int32) if fixed is not None else \
                    np.array([int(s['device_select']['index'][slot]) for s in sols], dtype=np.int32)
            got = _reduce_device(solver.ctxs[0], len(mine), n_mod, logp, log_quad, log_mix, log_prior, mode, pick, rows,
                                 B if pointwise else None, pointwise, keep_models, info)
            for le, e in enumerate(mine):
                outs[e] = _element_output(got, le, n_mod, delta, B, n_win, n_fun, pointwise, keep_models)
    finally:
        for entry in begun:
            if entry[3] is not None:            # (something failed before this launch was waited for: end it, it holds its solver)
                try:
                    entry[3]()
                except Exception:
                    pass
            entry[1]._lock.release()
    return outs, info


def _reduce_device(ctx, n_e, n_mod, logp, log_quad, log_mix, log_prior, mode, pick, rows, B, pointwise, keep_models, info):
    """``mxe_evidence_reduce`` over the elements of one device: per element a group of its models, scan e n_mod + m the
    chain of that index of the last launch"""
    off = np.arange(n_e + 1) * n_mod
    prior = None if log_prior is None else np.tile(log_prior, n_e)
    n_f = len(rows)
    t = {}
    want = ['mean', 'between'] + (['row'] if keep_models and pointwise and B is None else []) + \
        (['fval', 'fmean', 'fcov'] if n_f else [])
    common = dict(log_mix=log_mix, log_prior=prior, row_mode=mode, pick=pick, timing=t)
    red = ctx.evidence_reduce(off, logp, log_quad, F=rows if n_f else None, want=want, **common)
    info['reduce_ms'] += t.get('ms', 0.0)
    info['reduce_launches'] += 1
    out = dict(red, pick=pick, n_alpha=logp.shape[1])
    if pointwise and B is not None:
        # A = B H: the rows of B as functionals, a chunk at a time (the covariance block of a chunk is formed and dropped)
        Bm = np.asarray(B, dtype=float)
        nw = Bm.shape[0]
        A_mean, A_between = np.empty((n_e, nw)), np.empty((n_e, nw))
        A_models = np.empty((n_e * n_mod, nw)) if keep_models else None
        for c0 in range(0, nw, BLUR_CHUNK):
            c1 = min(c0 + BLUR_CHUNK, nw)
            part = ctx.evidence_reduce(off, logp, log_quad, F=Bm[c0:c1], want=('fval', 'fmean', 'fcov'), **common)
            info['reduce_ms'] += t.get('ms', 0.0)
            info['reduce_launches'] += 1
            A_mean[:, c0:c1] = part['fmean']
            A_between[:, c0:c1] = np.diagonal(part['fcov'], axis1=1, axis2=2)
            if keep_models:
                A_models[:, c0:c1] = part['fval']
        out.update(A_mean=A_mean, A_between=A_between, A_models=A_models)
    return out


def _element_output(got, le, n_mod, delta, B, n_win, n_fun, pointwise, keep_models):
    sl = slice(le * n_mod, (le + 1) * n_mod)
    logZ, w = got['logZ'][sl].copy(), got['wmodel'][sl].copy()
    kmax = got['kmax'][sl].astype(np.int64)
    usable = np.isfinite(logZ)
    with np.errstate(invalid='ignore'):
        out = dict(log_evidence=logZ, log_bayes_factor=logZ - (np.max(logZ[usable]) if usable.any() else np.nan),
                   weight=w, best=int(np.argmax(np.where(np.isfinite(w), w, -1.0))) if usable.any() else -1,
                   n_eff=float(1.0 / np.sum(w * w)) if np.sum(w * w) > 0 else np.nan,
                   alpha_index=kmax if got['pick'] is None else got['pick'][sl].astype(np.int64),
                   alpha_at_edge=(kmax == 0) | (kmax == got['n_alpha'] - 1),
                   n_good=got['ngood'][sl].astype(np.int64), n_used=int(got['used'][le]))
    if pointwise:
        if B is None:
            out['A'], out['A_model_err'] = got['mean'][le] / delta, np.sqrt(got['between'][le]) / delta
            if keep_models:
                out['A_models'] = got['row'][sl] / delta
        else:
            out['A'], out['A_model_err'] = got['A_mean'][le], np.sqrt(got['A_between'][le])
            if keep_models:
                out['A_models'] = got['A_models'][sl]
    nf = n_win + n_fun
    if nf:
        fmean, fcov, fval = got['fmean'][le], got['fcov'][le], got['fval'][sl]
        ferr = np.sqrt(np.diagonal(fcov))
        if n_win:
            out['window_weight'], out['window_err'], out['window_models'] = fmean[:n_win], ferr[:n_win], fval[:, :n_win]
        if n_fun:
            out['functional_value'], out['functional_err'] = fmean[n_win:], ferr[n_win:]
            out['functional_cov'], out['functional_models'] = fcov[n_win:, n_win:], fval[:, n_win:]
    return out


# ---- TauMaxEnt ---------------------------------------------------------------------------------------------------------

def _checked(loop, omega, models, prior):
    names, Ds = check_models(models, omega)
    log_prior = check_prior(prior, len(Ds))
    check_minimizer(loop)
    return names, Ds, log_prior


def tau_default_model_scan(tm, models, prior=None, alpha='bryan', windows=None, functionals=None, pointwise=True,
                           keep_models=True, timing=None):
    loop = tm.maxent_loop
    names, Ds, log_prior = _checked(loop, tm.omega, models, prior)
    choose_rows(alpha, loop.analyzers, len(loop.alpha_mesh))
    if loop.below_threshold():
        raise ValueError('default_model_scan: G is below the threshold, there is nothing to continue')
    template = loop.make_spec()
    ids = loop.device_ids if loop.device_ids else (loop.device_id,)
    outs, info = element_model_scan(tm.K, tm.omega, loop, [template], Ds, prior=log_prior, alpha=alpha, windows=windows,
                                    functionals=functionals, pointwise=pointwise, keep_models=keep_models,
                                    device_ids=ids[:1])
    out = outs[0]
    out['names'], out['info'] = names, info
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['reduce_ms'], kernel_ms=info['kernel_ms'], reduce_ms=info['reduce_ms'])
    return out


# ---- ElementwiseMaxEnt / DiagonalMaxEnt --------------------------------------------------------------------------------

def elementwise_default_model_scan(ew, models, prior=None, alpha='bryan', windows=None, functionals=None, pointwise=True,
                                   keep_models=True, timing=None):
    from .elementwise_maxent import DiagonalMaxEnt
    phases = [(ew.maxent_diagonal, ew._diag_jobs)]
    if not isinstance(ew, DiagonalMaxEnt):
        phases.append((ew.maxent_offdiagonal, ew._offdiag_jobs))
    checked = None
    for worker, _ in phases:
        checked = _checked(worker.maxent_loop, worker.omega, models, prior)
        choose_rows(alpha, worker.maxent_loop.analyzers, len(worker.maxent_loop.alpha_mesh))
    names, _, _ = checked
    ids = ew.device_ids if ew.device_ids else (ew.maxent_diagonal.maxent_loop.device_id,)
    collected = []
    info = dict(kernel_ms=0.0, reduce_ms=0.0, launches=0, reduce_launches=0, devices=[], n_elements=[])
    for worker, jobs_of in phases:
        loop = worker.maxent_loop
        _, Ds, log_prior = _checked(loop, worker.omega, models, prior)
        templates, keys = [], []
        for element, re in jobs_of():
            ew._load_element(worker, element, re)
            if loop.below_threshold():
                continue
            templates.append(loop.make_spec())
            keys.append(tuple(element) + (((0 if re else 1),) if ew.use_complex else ()))
        if not templates:
            continue
        outs, pinfo = element_model_scan(worker.K, worker.omega, loop, templates, Ds, prior=log_prior, alpha=alpha,
                                         windows=windows, functionals=functionals, pointwise=pointwise,
                                         keep_models=keep_models, device_ids=ids)
        for k in ('kernel_ms', 'reduce_ms', 'launches', 'reduce_launches'):
            info[k] += pinfo[k]
        info['devices'] = sorted(set(info['devices']) | set(pinfo['devices']))
        info['n_elements'].append(len(templates))
        if 'audit_max' in pinfo:
            info['audit_max'] = max(info.get('audit_max', 0.0), pinfo['audit_max'])
            info['audit_problems'] = info.get('audit_problems', 0) + pinfo.get('audit_problems', 0)
        collected.extend(zip(keys, outs))
    if not collected:
        raise ValueError('default_model_scan: every element is below the threshold')
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['reduce_ms'], kernel_ms=info['kernel_ms'], reduce_ms=info['reduce_ms'])
    # the layout of ElementwiseMaxEnt.resample_errors: matrix indices, then the complex index with use_complex
    struct = tuple(ew.shape) + ((2,) if ew.use_complex else ())
    out = dict(info=info, names=names)
    signed = ('A', 'A_models', 'window_weight', 'window_models', 'functional_value', 'functional_models')
    for key, o in collected:
        partner = (key[1], key[0]) + key[2:] if (ew.use_hermiticity and key[0] != key[1]) else None
        # G_ji = conj(G_ij): the same evidence and errors; the imaginary part's values change sign
        flip = -1.0 if (len(key) == 3 and key[2] == 1) else 1.0
        for name, val in o.items():
            val = np.asarray(val)
            if name not in out:
                out[name] = np.full(struct + val.shape, np.nan) if val.dtype.kind == 'f' else \
                    np.full(struct + val.shape, False if val.dtype.kind == 'b' else -1, dtype=val.dtype)
            out[name][key] = val
            if partner is not None:
                out[name][partner] = val * flip if (val.dtype.kind == 'f' and name in signed) else val
    return out
