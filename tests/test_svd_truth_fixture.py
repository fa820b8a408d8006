"""tests/golden/svd_truth.npz (make_golden_svd.py: adversarial matrices and their singular values from mpmath at 40
digits) is self-consistent, and the gates tests/test_gpu_svd_matrices.py holds the device decomposition to are fair:
LAPACK in binary64, the host backend, sits far inside every one of them.  No GPU, no mpmath."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = np.finfo(float).eps

SHAPES = {
    'graded_48x72': (48, 72), 'graded_64x96': (64, 96), 'graded_tall_72x48': (72, 48), 'odd_rank_40x60': (40, 60),
    'clustered_32x50': (32, 50), 'perm_diag_40x40': (40, 40), 'eye_40x40': (40, 40), 'rank3_dup_30x45': (30, 45),
    'one_row_1x37': (1, 37), 'one_col_37x1': (37, 1), 'one_by_one_1x1': (1, 1), 'narrow_5x3': (5, 3),
    'narrow_3x5': (3, 5), 'narrow_63x65': (63, 65), 'narrow_65x63': (65, 63), 'zeros_7x9': (7, 9),
}


@pytest.fixture(scope='module')
def tr():
    with np.load(os.path.join(GOLD, 'svd_truth.npz'), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


def test_the_fixture_holds_every_case_and_nothing_large(tr):
    assert sorted(str(n) for n in tr['names']) == sorted(SHAPES)
    assert os.path.getsize(os.path.join(GOLD, 'svd_truth.npz')) < os.path.getsize(os.path.join(GOLD, 'boson_kernels.npz'))
    for name, (m, n) in SHAPES.items():
        K, w, S = tr['K_' + name], tr['omega_' + name], tr['S_' + name]
        assert K.dtype == np.float64 and K.shape == (m, n) and np.all(np.isfinite(K))
        assert w.shape == (n,) and (n == 1 or np.all(np.diff(w) > 0))
        assert S.dtype == np.float64 and S.shape == (min(m, n),)


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_truth_is_sorted_and_lapack_agrees_within_four_eps(tr, name):
    K, S = tr['K_' + name], tr['S_' + name]
    assert np.all(S >= 0.0) and np.all(np.diff(S) <= 0.0)
    Sl = np.linalg.svd(K, compute_uv=False)
    d = np.abs(Sl - S).max()
    print('%s: LAPACK - truth %.2e = %.2f eps S_0' % (name, d, d / (EPS * S[0]) if S[0] > 0 else 0.0))
    assert d <= 4 * EPS * S[0]
    # (the truth is the 2-norm and the Frobenius norm of the matrix it belongs to)
    assert abs(np.sqrt((S.astype(np.longdouble) ** 2).sum()) - np.sqrt((K.astype(np.longdouble) ** 2).sum())) \
        <= 4 * EPS * max(S[0], 1e-300) * np.sqrt(len(S))
    if min(K.shape) == 1:
        assert abs(S[0] - float(np.sqrt((K.astype(np.longdouble) ** 2).sum()))) <= EPS * S[0]


def test_the_structure_of_each_case(tr):
    """what the table of make_golden_svd.py promises, read back from the truth"""
    for name in ('graded_48x72', 'graded_64x96', 'graded_tall_72x48'):
        S = tr['S_' + name]
        want = 10.0 ** np.linspace(1, -17, len(S))
        big = want >= 1e-12 * want[0]
        assert np.all(np.abs(S[big] - want[big]) <= 16 * EPS * want[0] + 1e-3 * want[big]), name
    S = tr['S_odd_rank_40x60']
    assert np.all(S[:33] > 1e-12 * S[0]) and np.all(S[33:] < 1e-15 * S[0])          # rank 33: odd
    S = tr['S_clustered_32x50']
    for i, v in enumerate((1.0, 1e-3, 1e-6)):
        assert np.all(np.abs(S[8 * i:8 * i + 8] - v) <= 16 * EPS), i
    assert np.all(S[24:] < 16 * EPS)
    assert np.array_equal(tr['S_perm_diag_40x40'], np.arange(40.0, 0.0, -1.0))
    assert np.array_equal(tr['S_eye_40x40'], np.ones(40)) and np.array_equal(tr['K_eye_40x40'], np.eye(40))
    K, S = tr['K_rank3_dup_30x45'], tr['S_rank3_dup_30x45']
    assert np.all(S[:3] > 1e-2 * S[0]) and np.all(S[3:] < 1e-15 * S[0])
    assert not K[:, 20].any() and not K[:, 44].any() and not K[13].any() and np.array_equal(K[:, 7], K[:, 3])
    assert not tr['K_zeros_7x9'].any() and not tr['S_zeros_7x9'].any()
