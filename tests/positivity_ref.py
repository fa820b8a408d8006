"""numpy restatement of ``mxe_hermitian_eig`` and of ``maxent_amd.positivity.matrix_positivity`` with
``numpy.linalg.eigh`` (LAPACK) on the same symmetrised matrices, the gate of the device kernel, and the matrix families
the device tests run.  Nothing here touches the device."""
import numpy as np

EPS = 2.0 ** -52
SIZES = (1, 2, 3, 5, 16, 17, 33, 64)
WAVE_M = 16                  # m <= this: one wavefront per matrix, four matrices per workgroup


def herm(A):
    A = np.asarray(A)
    return 0.5 * (A + np.conj(np.swapaxes(A, -1, -2)))


def fro(A):
    return np.sqrt(np.sum(np.abs(A) ** 2, axis=(-2, -1)))


def gate(m, lapack=0.0):
    """g(m) = 4 x max(LAPACK's own value of the same quantity on the same set, max(m, 8) 2^-52)"""
    return 4.0 * max(float(lapack), max(m, 8) * EPS)


def normalise(V):
    """columns of unit norm with the component of largest magnitude (lowest index on ties) real and positive"""
    V = np.array(V)
    for b in range(V.shape[0]):
        for k in range(V.shape[2]):
            v = V[b, :, k]
            i = int(np.argmax(np.abs(v)))
            v = v * (np.conj(v[i]) / np.abs(v[i])) / np.linalg.norm(v)
            V[b, :, k] = v
    return V


def pair_violation(H):
    """max over i < j of |h_ij| - sqrt(max(h_ii, 0) max(h_jj, 0)); 0 for a 1 x 1 matrix"""
    m = H.shape[-1]
    if m < 2:
        return np.zeros(H.shape[:-2])
    d = np.clip(np.real(np.einsum('...ii->...i', H)), 0.0, None)
    viol = np.abs(H) - np.sqrt(d[..., :, None] * d[..., None, :])
    iu = np.triu_indices(m, 1)
    return viol[..., iu[0], iu[1]].max(axis=-1)


def hermitian_eig_ref(A, floor=0.0):
    """what ``device.hermitian_eig`` returns for finite ``A`` (n_mat, m, m), from LAPACK"""
    A = np.asarray(A)
    H = herm(A)
    lam, V = np.linalg.eigh(H)
    V = normalise(V)
    lc = np.maximum(lam, floor)
    proj = np.einsum('bik,bk,bjk->bij', V, lc, np.conj(V))
    d = np.clip(floor - lam, 0.0, None)
    return dict(lam=lam, vec=V, proj=proj, neg=d.sum(axis=1), dist=np.sqrt((d ** 2).sum(axis=1)), pair=pair_violation(H),
                asym=fro(A - np.conj(np.swapaxes(A, -1, -2))), H=H, fro=fro(H))


def residuals(H, lam, V):
    """(|| H V - V Lambda ||_F / || H ||_F, || V^H V - I ||_F) per matrix; a zero matrix has residual 0"""
    R = np.einsum('bij,bjk->bik', H, V) - V * lam[:, None, :]
    n = fro(H)
    res = np.where(n > 0, fro(R) / np.where(n > 0, n, 1.0), fro(R))
    orth = fro(np.einsum('bji,bjk->bik', np.conj(V), V) - np.eye(V.shape[-1]))
    return res, orth


def trapezoid_delta(omega):
    w = np.asarray(omega, dtype=float)
    return 0.5 * np.concatenate(([w[1] - w[0]], w[2:] - w[:-2], [w[-1] - w[-2]]))


def positivity_ref(A, omega=None, delta=None, floor=0.0):
    """every quantity of ``matrix_positivity`` for ``A`` (M, M, n_omega) or (M, M, n_alpha, n_omega), from LAPACK"""
    A = np.asarray(A)
    M, n_omega = A.shape[0], A.shape[-1]
    if delta is None:
        delta = np.ones(n_omega) if omega is None else trapezoid_delta(omega)
    w = np.asarray(delta, dtype=float)
    lead = A.shape[2:]
    mats = np.moveaxis(A, (0, 1), (-2, -1)).reshape((-1, M, M))
    r = hermitian_eig_ref(mats, floor)
    lam = r['lam'].reshape(lead + (M,))
    out = dict(eigenvalues=lam, min_eigenvalue=lam[..., 0], eigenvectors=r['vec'].reshape(lead + (M, M)))
    out['negative_weight'] = np.dot(r['neg'].reshape(lead), w)
    out['trace_weight'] = np.dot(np.einsum('bii->b', r['H']).real.reshape(lead), w)
    out['negative_fraction'] = out['negative_weight'] / out['trace_weight']
    out['n_negative'] = np.sum(lam[..., 0] < floor - 2.0 * gate(M) * r['fro'].reshape(lead), axis=-1)
    pv = r['pair'].reshape(lead)
    out['pair_violation'] = pv
    proj = r['proj'].reshape(lead + (M, M))
    out['A_psd'] = np.moveaxis(proj, (-2, -1), (0, 1))
    out['distance'] = r['dist'].reshape(lead)
    out['trace_weight_psd'] = np.dot(np.einsum('...ii->...', proj).real, w)
    out['asymmetry'] = r['asym'].reshape(lead)
    out['fro'] = r['fro'].reshape(lead)
    return out


def compare_positivity(got, ref, M, delta):
    """``matrix_positivity`` against :func:`positivity_ref` within the gates of the kernel (LAPACK's own error taken as
    0: the bound is then the tighter one); ``delta``: the frequency weights.  Returns the worst ratio to a bound."""
    g = gate(M)
    n = ref['fro']
    worst = 0.0

    def check(name, err, bound):
        nonlocal worst
        ratio = float(np.max(err / bound)) if np.size(err) else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)

    tiny = np.finfo(float).tiny
    check('eigenvalues', np.abs(got['eigenvalues'] - ref['eigenvalues']), 2 * g * n[..., None] + tiny)
    check('A_psd', fro(np.moveaxis(got['A_psd'] - ref['A_psd'], (0, 1), (-2, -1))), 4 * g * n + tiny)
    check('distance', np.abs(got['distance'] ** 2 - ref['distance'] ** 2), 4 * g * n * n + tiny)
    check('pair_violation', np.abs(got['pair_violation'] - ref['pair_violation']), 4 * g * n + tiny)
    check('asymmetry', np.abs(got['asymmetry'] - ref['asymmetry']), 4 * g * (n + ref['asymmetry']) + tiny)
    # the frequency sums: per frequency at most M eigenvalues within 2 g || A ||_F each, and |tr dP| <= sqrt(M) || dP ||_F
    scale = 4 * g * M * np.dot(n, np.abs(np.asarray(delta, dtype=float))) + tiny
    for name in ('negative_weight', 'trace_weight', 'trace_weight_psd'):
        check(name, np.abs(np.asarray(got[name]) - np.asarray(ref[name])), scale)
    assert np.array_equal(got['n_negative'], ref['n_negative'])
    return worst


# ---- matrix families of the kernel tests ------------------------------------------------------------------------------------

def _rand(rng, shape, cplx):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if cplx else x


def _unitary(rng, n, m, cplx):
    q = np.linalg.qr(_rand(rng, (n, m, m), cplx))[0]
    return q


def _from_spectrum(rng, lam, cplx):
    """Q diag(lam) Q^H for random unitary Q; lam (n, m)"""
    n, m = lam.shape
    Q = _unitary(rng, n, m, cplx)
    return herm(np.einsum('bik,bk,bjk->bij', Q, lam, np.conj(Q)))


def families(m, cplx, n, seed=0):
    """name -> (n, m, m) matrices of every family the issue lists, real or complex"""
    rng = np.random.default_rng(1000 * m + (500 if cplx else 0) + seed)
    dt = complex if cplx else float
    eye = np.broadcast_to(np.eye(m, dtype=dt), (n, m, m)).copy()
    out = {}
    out['random'] = herm(_rand(rng, (n, m, m), cplx))
    d = np.zeros((n, m, m), dtype=dt)
    d[:, np.arange(m), np.arange(m)] = rng.standard_normal((n, m))
    out['diagonal'] = d
    out['identity'] = eye * rng.uniform(0.5, 2.0, (n, 1, 1)) * np.where(rng.random((n, 1, 1)) < 0.5, -1.0, 1.0)
    out['zero'] = np.zeros((n, m, m), dtype=dt)
    rep = np.repeat(rng.standard_normal((n, (m + 2) // 3)), 3, axis=1)[:, :m]
    out['repeated'] = _from_spectrum(rng, rep, cplx)
    v = _rand(rng, (n, m), cplx)
    out['rank_one'] = herm(np.einsum('bi,bj->bij', v, np.conj(v)))
    out['negative_definite'] = _from_spectrum(rng, -rng.uniform(0.1, 3.0, (n, m)), cplx)
    g = np.sign(rng.standard_normal((n, m))) * 10.0 ** np.linspace(-6, 6, m)[None, :] if m > 1 else np.ones((n, 1))
    out['wide_spectrum'] = _from_spectrum(rng, g, cplx)  # eigenvalues over 12 decades, mixed by a random unitary matrix
    s = 10.0 ** np.linspace(-3, 3, m) if m > 1 else np.ones(1)
    out['graded'] = out['random'] * s[None, :, None] * s[None, None, :]       # D H D: entries graded over 12 decades
    out['psd'] = _from_spectrum(rng, rng.uniform(0.0, 2.0, (n, m)), cplx)
    out['non_hermitian'] = _rand(rng, (n, m, m), cplx)
    if m >= 2:
        a = rng.uniform(0.5, 2.0, n)
        ph = np.exp(1j * rng.uniform(0, 2 * np.pi, n)) if cplx else np.where(rng.random(n) < 0.5, -1.0, 1.0)
        z = np.zeros((n, m, m), dtype=dt)
        z[:, 0, m - 1] = a * ph
        z[:, m - 1, 0] = a * np.conj(ph)
        out['zero_diagonal_pair'] = z                      # [[0, a e^{i phi}], [a e^{-i phi}, 0]] in the corners
    return out
