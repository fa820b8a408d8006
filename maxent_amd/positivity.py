"""Positivity of a matrix-valued spectral function (no counterpart in the reference).

A physical spectral function matrix A(omega) is Hermitian and positive semi-definite at every frequency.  Element-wise
continuation -- :class:`ElementwiseMaxEnt`, :class:`PoormanMaxEnt` -- usually does not give that (the reference's guide says
so; Poorman "usually improves" it).  This module says whether, where and by how much a result violates positivity, and
gives the nearest positive semi-definite spectrum and what that repair costs in chi2.

The work is one small Hermitian eigenproblem per frequency (and per alpha): ``mxe_hermitian_eig``, all matrices in one
launch.  Everything here is host glue around :func:`maxent_amd.device.hermitian_eig`; there is no CPU path for the
eigenproblem (``tests/positivity_ref.py`` is a numpy mirror for the tests).
"""

import numpy as np

from . import device as _dev

def accuracy_gate(m):
    """the bound on the relative residual and the orthogonality of the device's decomposition of an M x M matrix:
    4 x max(M, 8) x 2^-52; an eigenvalue is right to 2 x this x || A ||_F"""
    return 4.0 * max(int(m), 8) * 2.0 ** -52


def trapezoid_delta(omega):
    """the weights of :attr:`BaseOmegaMesh.delta` for any increasing array"""
    w = np.asarray(omega, dtype=float)
    if w.ndim != 1 or len(w) < 2:
        raise ValueError('positivity: omega must be one-dimensional with two points or more')
    return 0.5 * np.concatenate(([w[1] - w[0]], w[2:] - w[:-2], [w[-1] - w[-2]]))


def _weights(omega, delta, n_omega):
    if delta is None and omega is not None:
        delta = getattr(omega, 'delta', None)
        if delta is None:
            delta = trapezoid_delta(omega)
    if delta is None:
        return np.ones(n_omega)
    d = np.asarray(delta, dtype=float)
    if d.shape != (n_omega,):
        raise ValueError('positivity: %d frequency weights for %d frequencies' % (d.size, n_omega))
    return d


def matrix_positivity(A, omega=None, delta=None, floor=0.0, keep_vectors=False, device=0):
    """Is the matrix-valued spectral function ``A`` positive, and what is the nearest one that is?

    ``A``: (M, M, n_omega) or (M, M, n_alpha, n_omega), real or complex, from anywhere; M <= 64.  The frequency weights
    are ``delta``, else ``omega.delta``, else the trapezoid weights of the array ``omega``, else ones.  ``floor``: the
    smallest eigenvalue allowed (0: positive semi-definite).  One ``mxe_hermitian_eig`` launch for all frequencies and
    alphas on ``device``; the device works on the Hermitian part (A + A^H) / 2.

    Returns a dict; ``...`` stands for the alpha axis, where ``A`` has one:

    ``eigenvalues`` (..., n_omega, M) ascending, ``min_eigenvalue`` (..., n_omega), ``eigenvectors`` (..., n_omega, M, M;
    column k belongs to eigenvalue k) with ``keep_vectors``;
    ``negative_weight`` = sum_omega delta sum_{lambda < floor} (floor - lambda), ``trace_weight`` = sum_omega delta tr A,
    ``negative_fraction`` their ratio;
    ``n_negative``: the frequencies whose smallest eigenvalue lies below ``floor`` by more than the device's error bound,
    2 x ``accuracy_gate(M)`` x || A(omega) ||_F;
    ``pair_violation`` (..., n_omega) = max_{i<j} |A_ij| - sqrt(max(A_ii, 0) max(A_jj, 0)), positive where the necessary
    condition of the reference's guide fails, and ``worst_pair`` = (index of omega, i, j) of its largest value (with an
    alpha axis: an integer array (n_alpha, 3));
    ``A_psd`` (M, M, ..., n_omega): V max(Lambda, floor) V^H, the nearest matrix with eigenvalues >= floor in the Frobenius
    norm, exactly Hermitian, complex when ``A`` is; ``distance`` (..., n_omega) = || A_psd - Herm(A) ||_F;
    ``trace_weight_psd`` = sum_omega delta tr A_psd.  Clipping adds weight: the sum rule of ``A_psd`` is off by exactly
    ``negative_weight`` (for ``floor`` = 0), ``trace_weight_psd = trace_weight + negative_weight``; ``A_psd`` is not
    renormalised;
    ``asymmetry`` (..., n_omega) = || A - A^H ||_F of the input, ``sweeps`` (..., n_omega): the Jacobi sweeps of every
    matrix, ``info``: ``ms`` (device time of the kernel), ``n_matrices``, ``floor``.

    Raises ValueError for an ``A`` that is not finite (the message names an element) and MaxEntDeviceError if the
    iteration of a matrix did not end."""
    A = np.asarray(A)
    if A.ndim not in (3, 4) or A.shape[0] != A.shape[1]:
        raise ValueError('matrix_positivity: A must be (M, M, n_omega) or (M, M, n_alpha, n_omega); got %s' % (A.shape,))
    M, n_omega = A.shape[0], A.shape[-1]
    if not np.all(np.isfinite(A)):
        bad = np.argwhere(~np.isfinite(A))[0]
        raise ValueError('matrix_positivity: element (%d, %d) of A is not finite (first at index %s): was it continued?'
                         % (bad[0], bad[1], tuple(int(b) for b in bad[2:])))
    w = _weights(omega, delta, n_omega)
    lead = A.shape[2:]                                     # (n_alpha, n_omega) or (n_omega,)
    mats = np.ascontiguousarray(np.moveaxis(A, (0, 1), (-2, -1))).reshape((-1, M, M))
    t = {}
    want = ('lambda', 'proj', 'neg', 'dist', 'pair', 'asym') + (('vec',) if keep_vectors else ())
    got = _dev.hermitian_eig(mats, floor=floor, want=want, device=device, timing=t)
    if np.any(got['info'] < 0):
        k = int(np.flatnonzero(got['info'] < 0)[0])
        raise _dev.MaxEntDeviceError('matrix_positivity: matrix %s: mxe_hermitian_eig reports %d'
                                     % (np.unravel_index(k, lead), int(got['info'][k])))
    lam = got['lambda'].reshape(lead + (M,))
    out = dict(eigenvalues=lam, min_eigenvalue=lam[..., 0])
    if keep_vectors:
        out['eigenvectors'] = got['vec'].reshape(lead + (M, M))
    neg = got['neg'].reshape(lead)
    herm = 0.5 * (mats + np.conj(np.swapaxes(mats, 1, 2)))
    trace = np.einsum('kii->k', herm).real.reshape(lead)
    fro = np.sqrt(np.sum(np.abs(herm) ** 2, axis=(1, 2))).reshape(lead)
    out['negative_weight'] = _frequency_sum(neg, w)
    out['trace_weight'] = _frequency_sum(trace, w)
    with np.errstate(divide='ignore', invalid='ignore'):
        out['negative_fraction'] = out['negative_weight'] / out['trace_weight']
    out['n_negative'] = np.sum(lam[..., 0] < float(floor) - 2.0 * accuracy_gate(M) * fro, axis=-1)
    pv = got['pair'].reshape(lead)
    out['pair_violation'] = pv
    out['worst_pair'] = _worst_pair(herm.reshape(lead + (M, M)), pv)
    proj = got['proj'].reshape(lead + (M, M))
    out['A_psd'] = np.ascontiguousarray(np.moveaxis(proj, (-2, -1), (0, 1)))
    out['distance'] = got['dist'].reshape(lead)
    out['trace_weight_psd'] = _frequency_sum(np.einsum('...ii->...', proj).real, w)
    out['asymmetry'] = got['asym'].reshape(lead)
    out['sweeps'] = got['info'].reshape(lead)
    out['info'] = dict(ms=t.get('ms', 0.0), n_matrices=int(mats.shape[0]), floor=float(floor))
    return out


def _frequency_sum(x, w):
    """sum over omega of w x, every alpha by the same call: a row of an all-alpha answer has the bits of that alpha alone"""
    if x.ndim == 1:
        return np.dot(np.ascontiguousarray(x), w)
    return np.array([np.dot(np.ascontiguousarray(row), w) for row in x])


def _worst_pair(herm, pv):
    """(index of omega, i, j) of the largest pair violation; one row per alpha where there is an alpha axis"""
    def one(h, v):
        M = h.shape[-1]
        if M < 2:
            return (int(np.argmax(v)), 0, 0)
        k = int(np.argmax(v))
        d = np.clip(np.diagonal(h[k]).real, 0.0, None)
        viol = np.abs(h[k]) - np.sqrt(np.outer(d, d))
        iu = np.triu_indices(M, 1)
        b = int(np.argmax(viol[iu]))
        return (k, int(iu[0][b]), int(iu[1][b]))
    if pv.ndim == 1:
        return one(herm, pv)
    return np.array([one(herm[a], pv[a]) for a in range(pv.shape[0])], dtype=int)


# ---- ElementwiseMaxEnt / PoormanMaxEnt -----------------------------------------------------------------------------------

def _all_alphas(res, use_complex):
    """``res.A`` as (M, M, n_alpha, n_omega), complex where the job is, ``zero_elements`` as zeros"""
    A = np.array(res.A, dtype=float)
    for z in res.zero_elements:
        A[tuple(int(x) for x in z)] = 0.0
    return A[:, :, 0] + 1.0j * A[:, :, 1] if use_complex else A


def _matrix_of(ew, res, alpha):
    """(A (M, M, [n_alpha,] n_omega), the analyzer name or alpha index that was taken, None for all alphas) from the result
    of an element-wise job: the elements with their hermitian mirror, ``zero_elements`` as zeros"""
    from .resampling import choose_slot, SLOTS
    if isinstance(alpha, str) and alpha == 'all':
        A, which = _all_alphas(res, ew.use_complex), None
    else:
        slot, fixed = choose_slot(alpha, ew.maxent_diagonal.maxent_loop.analyzers, len(res.alpha))
        if fixed is None:
            A, which = np.array(res.get_A_out(SLOTS[slot])), SLOTS[slot]
        else:
            A, which = _all_alphas(res, ew.use_complex)[:, :, fixed], fixed
    if not np.all(np.isfinite(A)):
        bad = ~np.isfinite(A).reshape(A.shape[0], A.shape[1], -1).all(axis=2)
        i, j = (int(x) for x in np.argwhere(bad)[0])
        raise ValueError('positivity: element (%d, %d) of the result holds NaN: it was not continued (run() all elements, or '
                         'use hermiticity so that it follows from its partner)' % (i, j))
    return A, which


def elementwise_positivity(ew, result=None, alpha=None, floor=0.0, keep_vectors=False, back_continue=True):
    res = ew.run() if result is None else result
    A, which = _matrix_of(ew, res, alpha)
    ids = ew.device_ids if ew.device_ids else (ew.maxent_diagonal.maxent_loop.device_id,)
    out = matrix_positivity(A, delta=np.asarray(ew.maxent_diagonal.omega.delta, dtype=float), floor=floor,
                            keep_vectors=keep_vectors, device=ids[0])
    out['alpha'] = 'all' if which is None else which
    if back_continue and which is not None:
        out.update(_back_continue(ew, res, A, out['A_psd']))
    return out


def _back_continue(ew, res, A, A_psd):
    """per computed element: G_rec_psd = K_delta A_psd and chi2 of A and of A_psd in the element's own data space"""
    from . import posterior
    from .mock import check_job
    M = A.shape[0]
    ems = (M, M, 2) if ew.use_complex else (M, M)
    workers = [ew.maxent_diagonal, ew.maxent_offdiagonal]
    zero = set(tuple(int(x) for x in z) for z in res.zero_elements)
    done = {}
    for worker, jobs in zip(workers, (ew._diag_jobs(), ew._offdiag_jobs())):
        loop = worker.maxent_loop
        for element, re in jobs:
            cidx = 0 if re else 1
            key = tuple(element) + ((cidx,) if ew.use_complex else ())
            if key in zero:
                continue
            ew._load_element(worker, element, re)
            if loop.below_threshold():
                continue
            spec = loop.make_spec()
            posterior.check_alpha(spec, res.alpha)
            try:
                check_job(worker.K, spec, res.element_array('G_orig', key))
            except ValueError:
                raise ValueError('positivity: the result was not made from the data this object holds now (data were set '
                                 'since); run() again or hand in the result of the present job')
            Kd = np.asarray(worker.K.K_delta, dtype=float)
            G, err, T = np.asarray(spec['G_orig'], dtype=float), np.asarray(spec['err'], dtype=float), spec['T']
            part = (lambda x: x.real) if re else (lambda x: x.imag)
            rec = {}
            for name, X in (('', A), ('_psd', A_psd)):
                g = np.dot(Kd, np.asarray(part(X[element[0], element[1]]), dtype=float))
                r = g - G
                if T is not None:
                    r = np.dot(np.asarray(T), r)
                rec['chi2' + name] = float(np.sum(np.abs(r / err) ** 2))
                rec['G_rec' + name] = g
            done[key] = rec
    if not done:
        return {}
    n_rows = max(len(r['G_rec_psd']) for r in done.values())
    out = dict(G_rec_psd=np.full(ems + (n_rows,), np.nan), chi2=np.full(ems, np.nan), chi2_psd=np.full(ems, np.nan))
    for key, r in done.items():
        targets = [(key, 1.0)]
        if ew.use_hermiticity and key[0] != key[1]:        # (the partner follows from hermiticity: the same fit)
            targets.append(((key[1], key[0]) + key[2:], -1.0 if (len(key) == 3 and key[2] == 1) else 1.0))
        for k, sign in targets:
            if k != key and k in done:
                continue
            out['G_rec_psd'][k][:len(r['G_rec_psd'])] = sign * r['G_rec_psd']
            out['chi2'][k] = r['chi2']
            out['chi2_psd'][k] = r['chi2_psd']
    return out
