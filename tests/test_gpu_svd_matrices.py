"""The device SVD (svd_kernel of csrc/mxe_svd.hip.h, through device.kernel_svd_data) on matrices that are NOT one of
the smooth physical kernels: graded, rank deficient, clustered and repeated singular values, one row, one column,
wave-size edges, more rows than columns, the zero matrix, a batch whose items stop at different ranks, numerical rank
at and above the 128 rows the QR stage keeps, NaN and Inf.

Truth: tests/golden/svd_truth.npz, the singular values of each binary64 matrix from mpmath at 40 digits
(tests/golden/make_golden_svd.py; tests/test_svd_truth_fixture.py shows that LAPACK sits within 4 eps S_0 of it).
Gates: the ones the physical kernels are held to (test_gpu_iw.py, test_gpu_boson.py, test_gpu_api.py) --
|S - S_true| <= 1e-12 S_0, every true value >= 1e-12 S_0 returned, |U S V^T - K| <= 1e-13 ||K||_2, U and V
orthonormal to 1e-12 -- with the products taken in extended precision.  Where the only reference is LAPACK (no 40-digit
truth above 64 x 96) the gate on S is widened by LAPACK's own 4 eps S_0 and by nothing else.

``S`` non-increasing: equal neighbours are allowed (eye(40) has 40 equal values), an increase is not.

Each test prints what it measured (pytest -s); DESIGN.md 4l has the table of one run.
"""
import os

import numpy as np
import pytest

import maxent_amd as mx
from maxent_amd import device

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = np.finfo(float).eps
SVD_MAX_SWEEPS = 40              # csrc/mxe_svd.hip.h
SVD_RCAP = 128

CASES = ['graded_48x72', 'graded_64x96', 'graded_tall_72x48', 'odd_rank_40x60', 'clustered_32x50', 'perm_diag_40x40',
         'eye_40x40', 'rank3_dup_30x45', 'one_row_1x37', 'one_col_37x1', 'one_by_one_1x1', 'narrow_5x3', 'narrow_3x5',
         'narrow_63x65', 'narrow_65x63', 'zeros_7x9']


@pytest.fixture(scope='module')
def tr():
    with np.load(os.path.join(GOLD, 'svd_truth.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def svd_data(K, omega=None, **kw):
    """device.kernel_svd_data on a plain mesh (delta = 1: it serves the preblur only)"""
    n = K.shape[1]
    if omega is None:
        omega = np.linspace(-5.0, 5.0, n) if n > 1 else np.zeros(1)
    return device.kernel_svd_data(K, omega, np.ones(n), **kw)


def check(r, K, S_true, what, threshold=0.0, widen=0.0):
    """the gates of the module docstring on one result ``r`` for the matrix ``K`` whose singular values are ``S_true``
    (``widen``: the reference's own error in units of S_0, when ``S_true`` is LAPACK's)"""
    m, n = K.shape
    U, S, V = r['U'], r['S'], r['V']
    ns = len(S)
    S0 = S_true[0]
    assert S.shape == (ns,) and U.shape == (m, ns) and V.shape == (n, ns)             # exactly n_s columns
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(V))
    assert 0 < ns <= r['qr_rank'] <= min(m, n, SVD_RCAP)
    assert np.all(S > 0.0) and np.all(np.diff(S) <= 0.0) and np.all(S >= threshold)
    if r['qr_rank'] >= 2:
        assert 0 < r['sweeps'] < SVD_MAX_SWEEPS
    L = np.longdouble
    d_S = np.abs(S - S_true[:ns]).max() / S0
    # (values that must come back: every one >= 1e-12 S_0; under a threshold above that, every one above the
    #  threshold by more than the gate on S itself)
    k = int((S_true >= (1e-12 * S0 if threshold <= 1e-12 * S0 else threshold + 1e-12 * S0)).sum())
    d_K = np.abs((U.astype(L) * S.astype(L)) @ V.astype(L).T - K.astype(L)).max()
    # (with a threshold the product lacks the dropped directions: they count up to the first dropped true value)
    dropped = S_true[ns] if (threshold > 0.0 and ns < len(S_true)) else 0.0
    d_U = np.abs(U.astype(L).T @ U.astype(L) - np.eye(ns)).max()
    d_V = np.abs(V.astype(L).T @ V.astype(L) - np.eye(ns)).max()
    Sl = np.linalg.svd(K, compute_uv=False)
    d_lapack = np.abs(Sl[:ns] - S_true[:ns]).max() / S0
    print('SVDCASE %-34s thr %-7g n_s %3d qr_rank %3d sweeps %2d  |dS|/S_0 device %.2e LAPACK %.2e ratio %s  '
          '|USV^T-K|/S_0 %.2e  |U^TU-I| %.2e  |V^TV-I| %.2e'
          % (what, threshold, ns, r['qr_rank'], r['sweeps'], d_S, d_lapack,
             ('%.2f' % (d_S / d_lapack)) if d_lapack > 0 else ('inf' if d_S > 0 else '1'), float(d_K) / S0, float(d_U),
             float(d_V)))
    assert d_S <= 1e-12 + widen
    assert ns >= k
    assert d_K <= 1e-13 * S0 + dropped
    assert d_U <= 1e-12 and d_V <= 1e-12


# ---- 1. every fixture case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('threshold', [0.0, 1e-14])
@pytest.mark.parametrize('name', CASES)
def test_fixture_case_against_the_truth(tr, name, threshold):
    K, S_true = tr['K_' + name], tr['S_' + name]
    r = svd_data(K, tr['omega_' + name], threshold=threshold)[0]
    if name.startswith('zeros'):
        m, n = K.shape
        assert r['qr_rank'] == 0 and r['S'].shape == (0,) and r['U'].shape == (m, 0) and r['V'].shape == (n, 0)
        return
    check(r, K, S_true, name, threshold=threshold)
    if name.startswith('odd_rank') or name.startswith('rank3_dup'):
        rank = int((S_true >= 1e-12 * S_true[0]).sum())
        assert rank == (33 if name.startswith('odd_rank') else 3)
        assert np.all(r['S'][rank:] <= 1e-12 * S_true[0])             # (whatever is returned beyond the true rank is noise)


# ---- 2. threshold and ns_max --------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 5, 20, 30])
def test_threshold_and_ns_max_semantics(tr, i):
    """``threshold`` halfway (geometric mean) between the true values i and i + 1 of graded 48 x 72 (neighbours differ
    by 10**(18/47) = 2.4, the values are good to 1e-15 absolute): exactly i + 1 values; ``ns_max`` one short of that is
    status 2 / MXE_ERR_LIMIT, ``ns_max`` equal to it the bits of the default call"""
    K, S_true, w = tr['K_graded_48x72'], tr['S_graded_48x72'], tr['omega_graded_48x72']
    t = float(np.sqrt(S_true[i] * S_true[i + 1]))
    r = svd_data(K, w, threshold=t)[0]
    assert len(r['S']) == i + 1 and r['S'][-1] >= t
    check(r, K, S_true, 'graded_48x72 cut below value %d' % i, threshold=t)
    if i >= 1:
        with pytest.raises(device.MaxEntDeviceError, match='ns_max'):
            svd_data(K, w, threshold=t, ns_max=i)
    q = svd_data(K, w, threshold=t, ns_max=i + 1)[0]
    for key in ('U', 'S', 'V'):
        assert q[key].shape == r[key].shape and np.array_equal(q[key], r[key]), key
    assert (q['qr_rank'], q['sweeps']) == (r['qr_rank'], r['sweeps'])
    # the threshold is a cut on the result, not a parameter of the decomposition: the leading values of the full call
    full = svd_data(K, w, threshold=0.0)[0]
    assert np.array_equal(full['S'][:i + 1], r['S']) and np.array_equal(full['U'][:, :i + 1], r['U'])


# ---- 3. scaling by powers of two ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['graded_48x72', 'odd_rank_40x60', 'narrow_63x65', 'one_row_1x37'])
def test_scaling_by_a_power_of_two_changes_nothing_but_the_exponent_of_S(tr, name):
    """every cut of the kernel is relative (eps x the largest column norm, eps sqrt(aa bb)), square roots are taken of
    even powers, nothing under- or overflows: K 2**k gives the same U, V, rank and sweeps, and S 2**k, bit for bit"""
    K, w = tr['K_' + name], tr['omega_' + name]
    r0 = svd_data(K, w, threshold=0.0)[0]
    for k in (-100, 40, 100):
        r = svd_data(K * 2.0 ** k, w, threshold=0.0)[0]
        assert (r['qr_rank'], r['sweeps']) == (r0['qr_rank'], r0['sweeps']), k
        assert np.array_equal(r['S'], r0['S'] * 2.0 ** k), k
        assert np.array_equal(r['U'], r0['U']) and np.array_equal(r['V'], r0['V']), k


# ---- 4. the items of a batch --------------------------------------------------------------------------------------
def test_items_of_a_batch_that_stop_at_different_ranks_are_independent(tr):
    K, w = tr['K_graded_48x72'], tr['omega_graded_48x72']
    omega = mx.DataOmegaMesh(w)
    bs = [0.0, 0.3, 0.0, 1.5]
    res = device.kernel_svd_data(K, w, omega.delta, bs, threshold=0.0, want_K=True)
    print('batch: qr_rank %s n_s %s sweeps %s' % ([r['qr_rank'] for r in res], [len(r['S']) for r in res],
                                                 [r['sweeps'] for r in res]))
    # (the precondition of the test: the blur takes rank away, so the workgroups of one launch stop at different r)
    assert res[3]['qr_rank'] < res[1]['qr_rank'] < res[0]['qr_rank']
    for key in ('K', 'U', 'S', 'V'):
        assert np.array_equal(res[0][key], res[2][key]), key
    assert np.array_equal(res[0]['K'], K)
    for b, r in zip(bs, res):
        own = device.kernel_svd_data(K, w, omega.delta, [b], threshold=0.0, want_K=True)[0]
        for key in ('K', 'U', 'S', 'V'):
            assert own[key].shape == r[key].shape and np.array_equal(own[key], r[key]), (b, key)
        assert (own['qr_rank'], own['sweeps']) == (r['qr_rank'], r['sweeps'])
        Kd = K if b <= 0 else np.array(mx.PreblurKernel(K=mx.DataKernel(None, omega, K), b=b).K)
        assert np.abs(r['K'] - Kd).max() <= 1e-14 * np.linalg.norm(Kd, 2)
        # the decomposition of the matrix the device itself formed, against LAPACK on exactly that matrix
        check(r, r['K'], np.linalg.svd(r['K'], compute_uv=False), 'batch item b=%g' % b, widen=4 * EPS)


# ---- 5. transposition and fill edges ------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1), (1, 37), (37, 1), (31, 33), (33, 31), (32, 64), (65, 95)])
def test_transposition_returns_the_callers_bits(shape):
    m, n = shape
    K = np.random.RandomState(7000 + 100 * m + n).randn(m, n)
    r = svd_data(K, want_K=True, threshold=0.0)[0]
    assert r['K'].shape == K.shape and np.array_equal(r['K'], K)
    check(r, K, np.linalg.svd(K, compute_uv=False), 'transpose %dx%d' % shape, widen=4 * EPS)


class PlainMesh(object):
    """what the host kernels read of an omega mesh: its points and ``delta`` (ones: a one-point mesh has no spacing)"""

    def __init__(self, w):
        self._w = np.asarray(w, dtype=float)
        self.delta = np.ones(len(self._w))

    def __array__(self, dtype=None, copy=None):
        return self._w

    def __len__(self):
        return len(self._w)

    def __iter__(self):
        return iter(self._w)

    def __getitem__(self, i):
        return self._w[i]


@pytest.mark.parametrize('grid', [(1, 1), (3, 5), (17, 255), (16, 257)])
def test_fills_on_grids_that_are_no_multiple_of_the_block(grid):
    """element counts that are not a multiple of 256, one row, one column: the device fills equal the host fills under
    the gates of the existing tests (tau: 1e-15 absolute, test_gpu_api.py; Matsubara: 4e-16 max|K|, test_gpu_iw.py;
    bosonic tau: 16 eps max|K|, test_gpu_boson.py), and what the device decomposes is what it returned as K"""
    n_rows, n_w = grid
    beta = 10.0
    tau = np.linspace(0.0, beta, n_rows) if n_rows > 1 else np.array([beta / 3])
    iw = (2 * np.arange(n_rows) + 1) * np.pi / beta
    w = np.linspace(-8.0, 8.0, n_w) if n_w > 1 else np.array([0.7])
    omega, ones = PlainMesh(w), np.ones(n_w)
    for what, r, Kh, gate in (
            ('tau', device.kernel_svd(tau, w, ones, beta, want_K=True, threshold=0.0)[0],
             np.array(mx.TauKernel(tau, omega, beta=beta).K), 1e-15),
            ('iw', device.kernel_svd_iw(iw, w, ones, want_K=True, threshold=0.0)[0],
             np.array(mx.IOmegaKernel(iw, omega, beta=beta).K), None),
            ('boson', device.kernel_svd_boson(tau, w, ones, beta, want_K=True, threshold=0.0)[0],
             np.array(mx.BosonicTauKernel(tau, omega, beta=beta).K), None)):
        if gate is None:
            gate = (4e-16 if what == 'iw' else 16 * EPS) * np.abs(Kh).max()
        assert r['K'].shape == Kh.shape == ((2 * n_rows if what == 'iw' else n_rows), n_w)
        d = np.abs(r['K'] - Kh).max()
        print('fill %s %dx%d: max |K_dev - K_host| %.2e (gate %.2e)' % (what, n_rows, n_w, d, gate))
        assert np.all(np.isfinite(r['K'])) and d <= gate
        check(r, r['K'], np.linalg.svd(r['K'], compute_uv=False), 'fill %s %dx%d' % (what, n_rows, n_w), widen=4 * EPS)


# ---- 6. numerical rank at and above the cap ------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(200, 300), (129, 140)])
def test_more_than_128_significant_directions_are_refused(shape):
    """the QR stage keeps SVD_RCAP = 128 rows; the triplets of its rank-128 approximation are not the leading triplets
    of K.  Before status 3 existed the call returned them with MXE_OK; measured on the MI355X with that library: 200 x 300,
    128 values, up to 27.7 % off LAPACK's (median 6.2 %); 129 x 140, up to 8.2 %.  Now: an error that
    names the host backend."""
    K = np.random.RandomState(9000 + shape[0]).randn(*shape)
    with pytest.raises(device.MaxEntDeviceError, match='host'):
        r = svd_data(K, threshold=0.0)[0]
        Sl = np.linalg.svd(K, compute_uv=False)
        print('RANKCAP %dx%d returned: n_s %d, max |S - S_lapack| / S_lapack %.3e'
              % (shape + (len(r['S']), (np.abs(r['S'] - Sl[:len(r['S'])]) / Sl[:len(r['S'])]).max())))
    if shape == (200, 300):
        omega = mx.DataOmegaMesh(np.linspace(-5.0, 5.0, shape[1]))
        with pytest.raises(device.MaxEntDeviceError, match='host'):
            mx.DataKernel(None, omega, K, svd_backend='device').S


def test_rank_exactly_128_passes():
    """128 x 300 Gaussian: every row of R is needed and none is missing.  No 40-digit truth at this size: LAPACK, whose
    own error is below 4 eps S_0 (tests/test_svd_truth_fixture.py), and the gate on S widened by that"""
    K = np.random.RandomState(9128).randn(128, 300)
    r = svd_data(K, threshold=0.0)[0]
    assert r['qr_rank'] == 128 and len(r['S']) == 128
    check(r, K, np.linalg.svd(K, compute_uv=False), 'gaussian 128x300', widen=4 * EPS)
    # as many columns as the cap, more rows
    K = np.random.RandomState(9129).randn(140, 128)
    r = svd_data(K, threshold=0.0)[0]
    assert r['qr_rank'] == 128 and len(r['S']) == 128
    check(r, K, np.linalg.svd(K, compute_uv=False), 'gaussian 140x128', widen=4 * EPS)


# ---- 7. matrices that are not finite ------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_a_matrix_that_is_not_finite_does_not_return(bad):
    """before the check existed (measured with that library): MXE_OK and an EMPTY decomposition, n_s = 0 -- a NaN makes
    every comparison of the kernel false (qr_rank 20, nothing kept), an Inf stops the QR stage at its first step"""
    K = np.random.RandomState(77).randn(20, 30)
    K[7, 11] = bad
    with pytest.raises((device.MaxEntDeviceError, ValueError)):
        r = svd_data(K, threshold=0.0)[0]
        print('NONFINITE %r returned: n_s %d, S[:3] %s, NaN in S %s V %s'
              % (bad, len(r['S']), r['S'][:3], np.isnan(r['S']).any(), np.isnan(r['V']).any()))
    # the C entry point itself (without the wrapper's own check)
    w = np.linspace(-5.0, 5.0, 30)
    with pytest.raises(device.MaxEntDeviceError, match='finite'):
        device._kernel_svd_call('mxe_kernel_svd_data', 20, (device._p(np.ascontiguousarray(K)),), (), w, np.ones(30),
                                (0.0,), 0.0, 128, False, 0)


def test_squares_that_overflow_do_not_return_an_empty_decomposition():
    """a finite matrix whose squared column norms overflow stops the QR stage at its first step (inf > eps^2 inf is
    false); that is a numerical failure, not a matrix of rank 0"""
    K = np.random.RandomState(78).randn(20, 30) * 1e200
    with pytest.raises(device.MaxEntDeviceError, match='overflow'):
        svd_data(K, threshold=0.0)
