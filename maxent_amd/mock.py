"""Parametric bootstrap of a continuation (``TauMaxEnt.parametric_bootstrap``, ``ElementwiseMaxEnt.parametric_bootstrap``).
Not in the reference, whose users loop ``run()`` over mock data by hand.

For users without Monte Carlo bins -- a mean and error bars, or a mean and a covariance.  Mock data are drawn from the
continued spectrum with the noise of the job, G_k = K H0 + err o z_k in the data space of the job (the eigenbasis after
``set_cov``, the stacked real form of Matsubara data), and every mock is continued exactly like the data, with its own
alpha pick.  What is sampled is the distribution of the DATA under N(K H0, diag(err^2)) and what the whole procedure makes
of them; it is not a posterior.  The mean of what comes back minus what went in (``A_bias``) is what the procedure --
entropy, alpha selection, truncation -- does to this spectrum on average; the quantiles are bands that suit a positive,
skewed quantity; ``chi2_p_value`` says where the chi2 of the measured data lies among the chi2 of data that really came
from the continued spectrum.

The mocks of all sets of a job come from one ``mxe_mock_data`` call, the scans are the launch of
:func:`maxent_amd.resampling.element_resamples` (one per device, alpha picked on the device), mean, spread and the
quantile bands are taken there (``mxe_resample_reduce``, ``mxe_resample_quantiles``).  This module is the host glue and
the numpy mirror of the generator.  There is no CPU path.
"""

import numpy as np

from . import device, posterior
from .resampling import SIGNED, SLOTS, assemble_elements, check_minimizer, check_quantiles, choose_slot, element_resamples

#: alpha_mode of parametric_bootstrap -> alpha_mode of element_resamples
MODES = {'per_mock': 'per_resample', 'fixed': 'full_sample'}


# ---- host mirror, p-value (no device) ----------------------------------------------------------------------------------

def mock_rows(K, H0, err, seed, stream, n_mock, T=None, rank=None):
    """the host mirror of ``mxe_mock_data`` for one set: (n_mock, n_data) rows ``m + err * z[k]`` with m = K H0 (``T``
    given: the first ``rank`` rows of T applied to it) and ``z = posterior.sample_normals(seed, stream, n_mock, n_data)``,
    the generator's own mirror.  Row k depends on (seed, stream, k) alone, so fewer mocks are a prefix of more; an odd
    n_data cuts the last Box-Muller pair.  Rows >= rank are zeros.  The device agrees to rounding (it forms K H0 in
    another order and the normals with its own log, sin and cos), not to the bit."""
    K = np.asarray(K, dtype=float)
    m = np.dot(K, np.asarray(H0, dtype=float))
    n = len(m)
    r = n
    if (T is None) != (rank is None):
        raise ValueError('mock_rows: T and rank come together or not at all')
    if T is not None:
        r = int(rank)
        if not 0 <= r <= n:
            raise ValueError('mock_rows: rank {} outside 0..{}'.format(r, n))
        m = np.concatenate([np.dot(np.asarray(T, dtype=float)[:r], m), np.zeros(n - r)])
    e = np.asarray(err, dtype=float) * np.ones(n)
    z = posterior.sample_normals(seed, stream, n_mock, n)
    G = m[np.newaxis, :] + e[np.newaxis, :] * z
    G[:, r:] = 0.0
    return G


def chi2_p_value(chi2_obs, chi2_mock):
    """(1 + #{finite mock chi2 >= chi2_obs}) / (1 + #finite): the share of data sets drawn from the continued spectrum
    that fit as badly as the measured one or worse (never 0: the measured set counts as one of them).  Small: the
    measured data are not a typical draw -- error bars too small, correlations ignored, or a spectrum the kernel cannot
    carry.  It is conditional on the continued spectrum and says nothing about other spectra that fit.  NaN when
    ``chi2_obs`` is not finite."""
    obs = float(chi2_obs)
    if not np.isfinite(obs):
        return np.nan
    c = np.asarray(chi2_mock, dtype=float).ravel()
    c = c[np.isfinite(c)]
    return (1.0 + float(np.sum(c >= obs))) / (1.0 + len(c))


# ---- what the drivers share ---------------------------------------------------------------------------------------------

def check_arguments(loops, n_mock, seed, alpha_mode, quantiles):
    """refuse what needs no device to be refused; returns the quantiles as an array (or None)"""
    for loop in loops:
        check_minimizer(loop)
    if seed is None:
        raise ValueError('parametric_bootstrap: a seed is required (the mocks must be reproducible)')
    if n_mock is None or int(n_mock) < 2:
        raise ValueError('parametric_bootstrap: n_mock = {} (at least two are needed)'.format(n_mock))
    if alpha_mode not in MODES:
        raise ValueError("alpha_mode={!r}: 'per_mock' or 'fixed'".format(alpha_mode))
    return check_quantiles(quantiles, 'parametric', int(n_mock))


def check_job(K, spec, G_orig_result):
    """the result must have been made from the data the object holds now"""
    mine = np.asarray(K.fold(np.asarray(spec['G_orig'])))
    theirs = np.asarray(G_orig_result)
    if mine.shape != theirs.shape or not np.array_equal(mine, theirs):
        raise ValueError('parametric_bootstrap: the result was not made from the data this object holds now (data were set '
                         'since); run() again or hand in the result of the present job')


def _hidden_image(H, analysis, slot, fixed):
    i0 = fixed
    if i0 is None:
        try:
            i0 = int(analysis[SLOTS[slot]]['alpha_index'])
        except (KeyError, TypeError, IndexError):
            raise ValueError('parametric_bootstrap: the result has no {} to take the alpha from'.format(SLOTS[slot]))
    H0 = np.array(np.asarray(H, dtype=float)[i0])
    if not np.all(np.isfinite(H0)):
        raise ValueError('parametric_bootstrap: the spectrum at alpha index {} is not finite'.format(i0))
    return H0


def unrotated_matrix(K):
    """the matrix of kernel ``K`` without the left rotation it carries (with a PreblurKernel: blurred)"""
    inner = getattr(K, 'kernel', None)
    if inner is not None:
        return np.dot(unrotated_matrix(inner), K.B * np.asarray(K.omega.delta, dtype=float)[:, np.newaxis])
    if K.rotation is None and not getattr(K, '_projected', False):
        return np.asarray(K.K, dtype=float)
    Ku = getattr(K, '_K_unrotated', None)
    if Ku is None:
        raise NotImplementedError('parametric_bootstrap: this kernel does not keep its unrotated matrix')
    return np.asarray(Ku, dtype=float)


def _finish(o, n_mock, seed, G_mock):
    chi2 = o.pop('chi2_scans')
    o['chi2'], o['chi2_samples'] = float(chi2[0]), chi2[1:]
    o['chi2_p_value'] = chi2_p_value(chi2[0], chi2[1:])
    if 'A_mean' in o:
        o['A_bias'] = o['A_mean'] - o['A']
    o['n_mock'] = int(n_mock)
    if G_mock is not None:
        o['G_mock'] = G_mock
    return o


# ---- TauMaxEnt ---------------------------------------------------------------------------------------------------------

def tau_parametric_bootstrap(tm, result=None, n_mock=200, seed=None, alpha=None, alpha_mode='per_mock',
                             quantiles=(0.16, 0.5, 0.84), windows=None, functionals=None, pointwise=True, keep_samples=False,
                             keep_data=False, timing=None):
    loop = tm.maxent_loop
    q = check_arguments([loop], n_mock, seed, alpha_mode, quantiles)
    n_mock = int(n_mock)
    if result is None:
        result = tm.run()
    spec = loop.make_spec()
    posterior.check_alpha(spec, result.alpha)
    check_job(tm.K, spec, result.element_array('G_orig'))
    slot, fixed = choose_slot(alpha, loop.analyzers, len(spec['alpha']))
    H0 = _hidden_image(result.element_array('H'), result.analyzer_results, slot, fixed)
    ids = loop.device_ids if loop.device_ids else (loop.device_id,)
    t = {}
    # (the job's kernel as it stands -- rotated after set_cov, stacked, pre-blurred -- and the job's errors: its data space)
    got = device.mock_data(np.asarray(tm.K.K, dtype=float), H0[np.newaxis], spec['err'][np.newaxis], seed,
                           [posterior.stream_id(0, 0, 1, 0)], n_mock, device=ids[0], timing=t)
    G_rows = np.concatenate([np.asarray(spec['G'], dtype=float)[np.newaxis], got['G'][0]])
    outs, info = element_resamples(tm.K, tm.omega, loop, [spec], [G_rows], 'parametric', alpha=alpha,
                                   alpha_mode=MODES[alpha_mode], windows=windows, functionals=functionals, pointwise=pointwise,
                                   keep_samples=keep_samples, device_ids=ids[:1], quantiles=q)
    info['mock_ms'] = t.get('ms', 0.0)
    info['mock_bytes'] = int(got['G'].nbytes)
    info['left_out'] = info['left_out'].get(0, [])
    out = _finish(outs[0], n_mock, seed, got['G'][0] if keep_data else None)
    out['seed'] = int(seed)
    out['info'] = info
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['reduce_ms'] + info['mock_ms'], kernel_ms=info['kernel_ms'],
                      reduce_ms=info['reduce_ms'], mock_ms=info['mock_ms'])
    return out


# ---- ElementwiseMaxEnt / DiagonalMaxEnt --------------------------------------------------------------------------------

def _one_rotation(ph):
    """whether every element of the phase carries the same rotation object (or none)"""
    first = ph['templates'][0]['T']
    return all(s['T'] is first for s in ph['templates'])


def _phase_sets(ph, as_it_stands=None):
    """kernel matrix, errors, rotations and ranks of the sets of a phase in the form ``mxe_mock_data`` takes.  One rotation
    (or none) for every element -- ``set_error``, one ``set_cov`` for all --: the worker's kernel as it stands, no T.
    Rotations of their own (covariances per element): the unrotated kernel and T, rank per set.  ``as_it_stands``: the
    choice, made for the whole job (a phase of one element has one rotation, but must join the call of the other phase);
    default: this phase's own."""
    specs = ph['templates']
    if _one_rotation(ph) if as_it_stands is None else as_it_stands:
        return np.asarray(ph['worker'].K.K, dtype=float), np.stack([s['err'] for s in specs]), None, None
    Ku = unrotated_matrix(ph['worker'].K)
    n = Ku.shape[0]
    err, T, rank = np.ones((len(specs), n)), np.zeros((len(specs), n, n)), np.zeros(len(specs), dtype=np.int32)
    for s, spec in enumerate(specs):
        Ts = np.eye(n) if spec['T'] is None else np.asarray(spec['T'])
        if np.iscomplexobj(Ts):
            raise NotImplementedError('parametric_bootstrap: a complex rotation of the data space')
        r = Ts.shape[0]
        T[s, :r], rank[s], err[s, :r] = Ts, r, spec['err']
    return Ku, err, T, rank


def elementwise_parametric_bootstrap(ew, result=None, n_mock=200, seed=None, alpha=None, alpha_mode='per_mock',
                                     quantiles=(0.16, 0.5, 0.84), windows=None, functionals=None, pointwise=True,
                                     keep_samples=False, keep_data=False, timing=None):
    from .elementwise_maxent import DiagonalMaxEnt
    workers = [ew.maxent_diagonal] + ([] if isinstance(ew, DiagonalMaxEnt) else [ew.maxent_offdiagonal])
    q = check_arguments([w.maxent_loop for w in workers], n_mock, seed, alpha_mode, quantiles)
    n_mock = int(n_mock)
    res = ew.run() if result is None else result
    # a mirrored imaginary part is minus its partner: its quantile q is minus the partner's quantile 1 - q
    mirror = q is not None and ew.use_complex and ew.use_hermiticity and len(workers) == 2
    n_q = 0 if q is None else len(q)
    q_dev = np.concatenate([q, 1.0 - q]) if mirror else q
    zero = set(tuple(z) for z in res.zero_elements)
    phases = []
    for worker, jobs in zip(workers, (ew._diag_jobs(), ew._offdiag_jobs())):
        loop = worker.maxent_loop
        ph = dict(worker=worker, templates=[], keys=[], H0=[], streams=[])
        for element, re in jobs:
            cidx = 0 if re else 1
            key = tuple(element) + ((cidx,) if ew.use_complex else ())
            if key in zero:
                continue
            try:
                H = np.asarray(res.element_array('H', key), dtype=float)
            except (KeyError, IndexError, AttributeError, AssertionError):
                continue
            if H.ndim != 2 or H.shape[0] == 0:
                continue
            ew._load_element(worker, element, re)
            if loop.below_threshold():
                continue
            spec = loop.make_spec()
            posterior.check_alpha(spec, res.alpha)
            check_job(worker.K, spec, res.element_array('G_orig', key))
            slot, fixed = choose_slot(alpha, loop.analyzers, len(spec['alpha']))
            ana = res.analyzer_results
            for i in key:
                ana = ana[i]
            ph['templates'].append(spec)
            ph['keys'].append(key)
            ph['H0'].append(_hidden_image(H, ana, slot, fixed))
            ph['streams'].append(posterior.stream_id(int(np.ravel_multi_index(tuple(element), tuple(ew.shape))), cidx, 1, 0))
        if ph['templates']:
            phases.append(ph)
    if not phases:
        raise ValueError('parametric_bootstrap: the result holds no element to draw mocks from')
    as_it_stands = all(_one_rotation(ph) for ph in phases)
    for ph in phases:                                     # (the workers are two objects: each still holds its last element)
        ph['K'], ph['err'], ph['T'], ph['rank'] = _phase_sets(ph, as_it_stands)
    ids = ew.device_ids if ew.device_ids else (ew.maxent_diagonal.maxent_loop.device_id,)
    # one mxe_mock_data call for all sets of the job where the phases share the kernel matrix (they do unless the workers
    # were given different kernels), else one per phase
    calls = [[ph] for ph in phases]
    if len(phases) == 2 and (phases[0]['T'] is None) == (phases[1]['T'] is None) and \
            phases[0]['K'].shape == phases[1]['K'].shape and np.array_equal(phases[0]['K'], phases[1]['K']):
        calls = [phases]
    info = dict(kernel_ms=0.0, reduce_ms=0.0, mock_ms=0.0, mock_bytes=0, mock_calls=len(calls), launches=0, reduce_launches=0,
                n_datasets=[], n_elements=[], left_out={})
    for group in calls:
        t = {}
        cat = lambda name: None if group[0][name] is None else np.concatenate([ph[name] for ph in group])
        got = device.mock_data(group[0]['K'], np.concatenate([np.stack(ph['H0']) for ph in group]), cat('err'), seed,
                               sum((ph['streams'] for ph in group), []), n_mock, T=cat('T'), rank=cat('rank'), device=ids[0],
                               timing=t)
        info['mock_ms'] += t.get('ms', 0.0)
        info['mock_bytes'] += int(got['G'].nbytes)
        s = 0
        for ph in group:
            ph['G'] = got['G'][s:s + len(ph['templates'])]
            s += len(ph['templates'])
    collected = []
    for ph in phases:
        worker = ph['worker']
        G_rows = [np.concatenate([np.asarray(spec['G'], dtype=float)[np.newaxis], ph['G'][e][:, :len(spec['G'])]])
                  for e, spec in enumerate(ph['templates'])]
        outs, pinfo = element_resamples(worker.K, worker.omega, worker.maxent_loop, ph['templates'], G_rows, 'parametric',
                                        alpha=alpha, alpha_mode=MODES[alpha_mode], windows=windows, functionals=functionals,
                                        pointwise=pointwise, keep_samples=keep_samples, device_ids=ids, quantiles=q_dev)
        info['kernel_ms'] += pinfo['kernel_ms']
        info['reduce_ms'] += pinfo['reduce_ms']
        info['launches'] += pinfo['launches']
        info['reduce_launches'] += pinfo['reduce_launches']
        info['n_datasets'].append(pinfo['n_datasets'])
        info['n_elements'].append(len(ph['templates']))
        if 'audit_max' in pinfo:
            info['audit_max'] = max(info.get('audit_max', 0.0), pinfo['audit_max'])
        for e, lo in pinfo['left_out'].items():
            info['left_out'][ph['keys'][e]] = lo
        for e, o in enumerate(outs):
            G_mock = ph['G'][e][:, :len(ph['templates'][e]['G'])] if keep_data else None
            collected.append((ph['keys'][e], _finish(o, n_mock, seed, G_mock)))
    if timing is not None:
        timing.update(ms=info['kernel_ms'] + info['reduce_ms'] + info['mock_ms'], kernel_ms=info['kernel_ms'],
                      reduce_ms=info['reduce_ms'], mock_ms=info['mock_ms'])
    return _assemble(ew, collected, dict(info=info, method='parametric', n_mock=n_mock, seed=int(seed)), q, n_q, mirror)


def _assemble(ew, collected, out, q, n_q, mirror):
    """the layout of ``elementwise_resample_errors`` (``resampling.assemble_elements``); ``G_mock`` is a signed value too,
    padded with NaN to the longest element (covariances per element keep different numbers of data rows)"""
    if q is not None:
        out['quantiles'] = np.array(q)
    out['n_resamples'] = out['n_mock']
    if any('G_mock' in o for _, o in collected):
        longest = max(o['G_mock'].shape[-1] for _, o in collected)
        for _, o in collected:
            o['G_mock'] = np.pad(o['G_mock'], [(0, 0), (0, longest - o['G_mock'].shape[-1])], constant_values=np.nan)
    return assemble_elements(ew, collected, out, n_q, mirror, shared=('method', 'n_resamples', 'n_mock', 'quantiles'),
                             signed=SIGNED + ('G_mock',))
