"""``mxe_hermitian_eig`` (device.hermitian_eig) against ``numpy.linalg.eigh`` on the same symmetrised matrices.

The gate, per size m and set of matrices: g = 4 x max(LAPACK's own value of the same quantity on the same set,
max(m, 8) 2^-52) -- the factor 4 is the project's gate for its other Jacobi code.  Required of every matrix:
|| Herm(A) V - V Lambda ||_F / || A ||_F <= g, || V^H V - I ||_F <= g, |lambda - lambda_ref| <= 2 g || A ||_F (Weyl),
|| A_psd - A_psd_ref ||_F <= 4 g || A ||_F (the projection onto the cone does not expand), out_dist^2 and out_neg within
4 g || A ||_F^2 and 4 g || A ||_F; no matrix may report -2, and at most 30 sweeps.

Measured on an MI355X (test_families prints its own per m; the table is in DESIGN.md, section 4x), worst over all
families in units of max(m, 8) 2^-52, where the gate is 4: residual 0.35 (m = 2), 0.56 (3), 0.85 (5), 2.24 (16), 1.50 (17),
1.38 (33), 2.11 (64) beside LAPACK's 0.12 to 0.54; orthogonality 0.23 to 0.56 beside LAPACK's 0.18 to 1.37; at most 16
sweeps (m = 64), none exhausted."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from maxent_amd import device
import positivity_ref as R

pytestmark = pytest.mark.gpu

N_PER_FAMILY = 7
_RUNS = {}


def _run(m, cplx):
    """every family at size m, each one device call of N_PER_FAMILY matrices, and its LAPACK mirror; computed once"""
    key = (m, cplx)
    if key not in _RUNS:
        out = {}
        for name, X in R.families(m, cplx, N_PER_FAMILY).items():
            out[name] = (X, device.hermitian_eig(X), R.hermitian_eig_ref(X))
        _RUNS[key] = out
    return _RUNS[key]


def _check_against_lapack(m, X, got, ref, what, floor=0.0):
    """the gates of the module docstring; returns (residual, orthogonality, LAPACK's residual, LAPACK's orthogonality,
    largest sweep count)"""
    n = ref['fro']
    assert got['info'].dtype == np.int32 and np.all(got['info'] >= 0) and np.all(got['info'] <= device.HERMEIG_MAX_SWEEPS), \
        (what, got['info'])
    res, orth = R.residuals(ref['H'], got['lambda'], got['vec'])
    res_l, orth_l = R.residuals(ref['H'], ref['lam'], ref['vec'])
    g_res, g_orth = R.gate(m, res_l.max()), R.gate(m, orth_l.max())
    g = max(g_res, g_orth)
    tiny = np.finfo(float).tiny
    assert res.max() <= g_res, (what, 'residual', res.max(), g_res)
    assert orth.max() <= g_orth, (what, 'orthogonality', orth.max(), g_orth)
    assert np.all(np.diff(got['lambda'], axis=1) >= 0), what
    assert np.all(np.abs(got['lambda'] - ref['lam']) <= 2 * g * n[:, None] + tiny), (what, 'lambda')
    assert np.all(R.fro(got['proj'] - ref['proj']) <= 4 * g * n + tiny), (what, 'proj')
    assert np.all(np.abs(got['dist'] ** 2 - ref['dist'] ** 2) <= 4 * g * n * (n + abs(floor) * np.sqrt(m)) + tiny), (what, 'dist')
    assert np.all(np.abs(got['neg'] - ref['neg']) <= 4 * g * n + tiny), (what, 'neg')
    # the projection is Hermitian to the bit, the eigenvectors are normalised like those of mxe_bins_eig
    assert np.array_equal(got['proj'], np.conj(np.swapaxes(got['proj'], 1, 2))), what
    V = got['vec']
    # (a component of largest magnitude -- to rounding, which may order near-ties differently here -- is real and positive)
    cand = (V.imag == 0.0) & (V.real > 0.0) & (np.abs(V) >= (1 - 4 * R.EPS) * np.abs(V).max(axis=1, keepdims=True))
    assert np.all(cand.any(axis=1)), what
    assert np.all(np.abs(np.linalg.norm(V, axis=1) - 1.0) <= max(m, 8) * R.EPS), what
    # the two quantities that are formed from the entries alone
    assert np.all(np.abs(got['pair'] - ref['pair']) <= 8 * R.EPS * n + tiny), (what, 'pair')
    # (a sum of m^2 squares in some order: at most m^2 2^-53 relative, half of it after the root; a few roundings per term)
    assert np.all(np.abs(got['asym'] - ref['asym']) <= (m * m / 4 + 4) * R.EPS * ref['asym'] + tiny), (what, 'asym')
    return res.max(), orth.max(), res_l.max(), orth_l.max(), int(got['info'].max())


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', R.SIZES)
def test_families(m, cplx):
    worst = [0.0, 0.0, 0.0, 0.0, 0]
    for name, (X, got, ref) in _run(m, cplx).items():
        assert got['vec'].dtype == X.dtype and got['proj'].dtype == X.dtype and got['lambda'].shape == (N_PER_FAMILY, m)
        r = _check_against_lapack(m, X, got, ref, (m, cplx, name))
        worst = [max(a, b) for a, b in zip(worst, r)]
    u = max(m, 8) * R.EPS
    print('m = %2d %s: residual %.2f (LAPACK %.2f), orthogonality %.2f (LAPACK %.2f) in units of max(m, 8) 2^-52; '
          'largest sweep count %d' % (m, 'complex' if cplx else 'real', worst[0] / u, worst[2] / u, worst[1] / u, worst[3] / u,
                                      worst[4]))


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', R.SIZES)
def test_matrices_with_nothing_to_rotate(m, cplx):
    run = _run(m, cplx)
    for name in ('diagonal', 'identity', 'zero'):
        X, got, ref = run[name]
        assert np.all(got['info'] == 0), name
        d = np.real(np.einsum('bii->bi', X))
        assert np.array_equal(got['lambda'], np.sort(d, axis=1)), name               # the diagonal itself, sorted
        assert np.all(np.sort(np.abs(got['vec']).reshape(len(X), -1), axis=1)[:, -m:] == 1.0), name
        assert np.all(np.sum(got['vec'] != 0, axis=(1, 2)) == m), name                # a permutation matrix
        assert np.all(got['asym'] == 0.0), name
    assert np.all(run['zero'][1]['proj'] == 0.0) and np.all(run['zero'][1]['dist'] == 0.0)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', [s for s in R.SIZES if s >= 2])
def test_vanishing_diagonals_with_a_finite_off_diagonal(m, cplx):
    """[[0, a e^{i phi}], [a e^{-i phi}, 0]]: its columns are orthogonal, a one-sided sweep would do nothing"""
    X, got, ref = _run(m, cplx)['zero_diagonal_pair']
    a = np.abs(X[:, 0, m - 1])
    g = R.gate(m)
    assert np.all(got['info'] >= 1)
    assert np.all(np.abs(got['lambda'][:, 0] + a) <= 2 * g * ref['fro']) and np.all(np.abs(got['lambda'][:, -1] - a) <= 2 * g * ref['fro'])
    assert np.all(np.abs(got['lambda'][:, 1:-1]) <= 2 * g * ref['fro'][:, None])
    assert np.all(np.abs(got['pair'] - a) <= 8 * R.EPS * a) and np.all(np.abs(got['neg'] - a) <= 4 * g * ref['fro'])


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', R.SIZES)
def test_psd_comes_back_and_the_projection_is_idempotent(m, cplx):
    run = _run(m, cplx)
    g = R.gate(m)
    X, got, ref = run['psd']
    assert np.all(R.fro(got['proj'] - ref['H']) <= 4 * g * ref['fro']) and np.all(got['dist'] <= 4 * g * ref['fro'])
    for name in ('random', 'negative_definite', 'wide_spectrum'):
        X, got, ref = run[name]
        again = device.hermitian_eig(got['proj'], want=('proj', 'neg', 'lambda'))
        n = R.fro(got['proj'])
        assert np.all(again['info'] >= 0), name
        assert np.all(R.fro(again['proj'] - got['proj']) <= 4 * g * n + np.finfo(float).tiny), name
        assert np.all(again['lambda'] >= -2 * g * n[:, None]), name
    assert np.all(run['negative_definite'][1]['lambda'] < 0)
    assert np.all(R.fro(run['negative_definite'][1]['proj']) <= 4 * g * run['negative_definite'][2]['fro'])


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', [3, 16, 33])
def test_a_non_hermitian_input_is_its_hermitian_part(m, cplx):
    X, got, ref = _run(m, cplx)['non_hermitian']
    assert np.all(got['asym'] > 0)
    same = device.hermitian_eig(ref['H'])
    for name in ('lambda', 'vec', 'proj', 'neg', 'dist', 'pair', 'info'):
        assert np.array_equal(got[name], same[name]), name                # (A + A^H) / 2 is formed the same way: the same bits
    assert np.all(same['asym'] == 0.0)


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', [5, 16, 17, 64])
def test_floor_and_the_outputs_asked_for(m, cplx):
    X = _run(m, cplx)['random'][0]
    floor = 0.25
    got = device.hermitian_eig(X, floor=floor)
    _check_against_lapack(m, X, got, R.hermitian_eig_ref(X, floor), (m, cplx, 'floor'), floor=floor)
    only = device.hermitian_eig(X, floor=floor, want=('neg',))
    assert sorted(only) == ['info', 'neg'] and np.array_equal(only['neg'], got['neg']) and np.array_equal(only['info'], got['info'])
    one = device.hermitian_eig(X[2], floor=floor)
    assert one['lambda'].shape == (m,) and one['proj'].shape == (m, m) and one['info'].shape == ()
    for name in got:
        assert np.array_equal(one[name], got[name][2]), name


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', [2, 5, 16, 17, 33])
def test_the_same_bits_alone_in_a_batch_and_again(m, cplx):
    """n_mat = 1, 7 and one more than a multiple of the matrices per workgroup (four for m <= 16, one above): the grid's
    tail; a matrix's bits depend on nothing but the matrix"""
    n = 4 * 3 + 1
    X = R.families(m, cplx, n, seed=5)['random']
    X[1] = R.families(m, cplx, 1, seed=6)['wide_spectrum'][0]                  # neighbours that take other numbers of sweeps
    X[n - 1] = R.families(m, cplx, 1, seed=7)['repeated'][0]
    full = device.hermitian_eig(X)
    assert np.all(full['info'] >= 0)
    print('m = %d: sweeps of the batch %s' % (m, full['info'].tolist()))
    again = device.hermitian_eig(X)
    seven = device.hermitian_eig(X[:7])
    for name in full:
        assert np.array_equal(full[name], again[name]), name
        assert np.array_equal(full[name][:7], seven[name]), name
    for k in (0, 1, 5, n - 1):
        alone = device.hermitian_eig(X[k:k + 1])
        for name in full:
            assert np.array_equal(full[name][k:k + 1], alone[name]), (name, k)
    _check_against_lapack(m, X, full, R.hermitian_eig_ref(X), (m, cplx, 'batch'))


@pytest.mark.parametrize('cplx', [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize('m', [3, 16, 17])
def test_a_nan_matrix_among_good_ones(m, cplx):
    X = R.families(m, cplx, 7, seed=9)['random']
    clean = device.hermitian_eig(X)
    for bad_value, k in ((np.nan, 2), (np.inf, 6)):
        Y = X.copy()
        Y[k, m - 1, 0] = bad_value
        got = device.hermitian_eig(Y)
        assert got['info'][k] == -1
        for name in got:
            if name == 'info':
                continue
            assert np.all(np.isnan(got[name][k])), name
            keep = np.arange(7) != k
            assert np.array_equal(got[name][keep], clean[name][keep]), name          # bitwise what they are without it
        assert np.array_equal(got['info'][keep], clean['info'][keep])


def test_beyond_the_cap_nothing_is_written():
    lib = device.load_library()
    m = device.HERMEIG_MAX_M + 1
    A = np.eye(m)
    sentinel = -12345.0
    outs = [np.full(s, sentinel) for s in ((m,), (m, m), (m, m), (1,), (1,), (1,), (1,))]
    info = np.full(1, 77, dtype=np.int32)
    ms = ctypes.c_float(-1.0)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.mxe_hermitian_eig(0, 1, m, 0, A.ctypes.data_as(dp), 0.0, *([o.ctypes.data_as(dp) for o in outs] +
                               [info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms)]))
    assert rc == -5                                                        # MXE_ERR_LIMIT
    assert all(np.all(o == sentinel) for o in outs) and info[0] == 77 and ms.value == -1.0
    for args in ((0, 3, 0), (1, 0, 0), (1, 3, 2)):                         # n_mat < 1, m < 1, is_complex outside {0, 1}
        assert lib.mxe_hermitian_eig(0, args[0], args[1], args[2], A.ctypes.data_as(dp), 0.0, *([o.ctypes.data_as(dp) for o in outs] +
                                     [info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms)])) == -1
    assert lib.mxe_hermitian_eig(0, 1, 3, 0, A.ctypes.data_as(dp), float('nan'), *([o.ctypes.data_as(dp) for o in outs] +
                                 [info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(ms)])) == -1
    assert all(np.all(o == sentinel) for o in outs) and info[0] == 77
    # every output pointer may be NULL
    assert lib.mxe_hermitian_eig(0, 1, 3, 0, A.ctypes.data_as(dp), 0.0, None, None, None, None, None, None, None, None, None) == 0
