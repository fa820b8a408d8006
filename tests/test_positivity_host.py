"""Positivity of a matrix-valued A, the part that needs no GPU: the entry point is declared, the refusals that come before
the device is touched, and the numpy mirror (tests/positivity_ref.py) on the reference's own outputs -- the numbers the
feature was asked for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxent_amd as mx
from maxent_amd import device, positivity
import positivity_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def test_the_entry_point_is_declared():
    names = [s[0] for s in device.SYMBOLS]
    header = open(os.path.join(ROOT, 'include', 'maxent_hip.h')).read()
    assert 'mxe_hermitian_eig' in names and 'int  mxe_hermitian_eig(' in header
    assert '#define MXE_HERMEIG_MAX_M      64' in header and device.HERMEIG_MAX_M == 64
    source = open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'maxent_hip.hip')).read()
    assert 'extern "C" int mxe_hermitian_eig(' in source and '#include "mxe_hermeig.hip.h"' in source
    hdr = [line for line in open(os.path.join(ROOT, 'maxent_amd', 'csrc', 'Makefile')) if line.startswith('HDR')]
    assert len(hdr) == 1 and 'mxe_hermeig.hip.h' in hdr[0].split()
    assert mx.matrix_positivity is positivity.matrix_positivity
    for cls in (mx.ElementwiseMaxEnt, mx.DiagonalMaxEnt, mx.PoormanMaxEnt):
        assert callable(getattr(cls, 'positivity'))
    assert mx.PoormanMaxEnt.positivity is mx.ElementwiseMaxEnt.positivity


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(device, 'load_library', refuse)
    monkeypatch.setattr(device, 'device_count', refuse)


@pytest.mark.parametrize('A,kw', [
    (np.zeros((3, 2)), {}),                                  # not square
    (np.zeros((4, 3, 2)), {}),
    (np.zeros(5), {}),
    (np.zeros((2, 2, 2, 2)), {}),
    (np.zeros((0, 3, 3)), {}),                               # n_mat < 1
    (np.zeros((2, 0, 0)), {}),                               # m < 1
    (np.zeros((1, 65, 65)), {}),                             # beyond MXE_HERMEIG_MAX_M
    (np.zeros((2, 2), dtype=object), {}),
    (np.eye(3), dict(floor=np.nan)),
    (np.eye(3), dict(floor=np.inf)),
    (np.eye(3), dict(floor='low')),
    (np.eye(3), dict(want=('lambda', 'vectors'))),
])
def test_hermitian_eig_refuses_before_the_library(no_library, A, kw):
    with pytest.raises(ValueError):
        device.hermitian_eig(A, **kw)


def test_hermitian_eig_refuses_sizes_beyond_int32(no_library):
    # 2^31 numbers: a view without memory behind it
    A = np.lib.stride_tricks.as_strided(np.zeros(1), shape=(2 ** 19, 64, 64), strides=(0, 0, 0))
    with pytest.raises(ValueError, match='2\\^31'):
        device.hermitian_eig(A)
    with pytest.raises(ValueError, match='2\\^31'):
        device.hermitian_eig(np.lib.stride_tricks.as_strided(np.zeros(1, dtype=complex), shape=(2 ** 18, 64, 64), strides=(0, 0, 0)))


def test_matrix_positivity_refuses_before_the_library(no_library):
    with pytest.raises(ValueError):
        mx.matrix_positivity(np.zeros((2, 3, 10)))
    with pytest.raises(ValueError):
        mx.matrix_positivity(np.zeros((2, 2)))
    A = np.zeros((2, 2, 10))
    A[0, 1, 4] = np.nan
    with pytest.raises(ValueError, match=r'element \(0, 1\)'):
        mx.matrix_positivity(A)
    with pytest.raises(ValueError, match='weights'):
        mx.matrix_positivity(np.zeros((2, 2, 10)), delta=np.ones(9))


def test_diagonal_maxent_refuses():
    with pytest.raises(NotImplementedError, match='off-diagonal'):
        mx.DiagonalMaxEnt().positivity()


def test_the_mirror_gives_the_numbers_of_the_reference_outputs():
    g = np.load(os.path.join(GOLD, 'elementwise.npz'))
    assert np.array_equal(R.trapezoid_delta(g['omega']), positivity.trapezoid_delta(g['omega']))
    np.testing.assert_allclose(positivity.trapezoid_delta(g['omega']), g['delta'], rtol=1e-14)
    ew = R.positivity_ref(g['ew_A_out'], delta=g['delta'])
    pm = R.positivity_ref(g['pm_A_out'], delta=g['delta'])
    assert ew['n_negative'] == 68 and pm['n_negative'] == 67
    assert abs(ew['min_eigenvalue'].min() + 0.194) < 5e-4 and abs(pm['min_eigenvalue'].min() + 0.0146) < 5e-5
    assert abs(ew['negative_weight'] - 0.1188) < 5e-5 and abs(pm['negative_weight'] - 0.00959) < 5e-6
    assert abs(ew['trace_weight'] - 1.9972) < 5e-5 and abs(pm['trace_weight'] - 1.9972) < 5e-5
    assert abs(ew['negative_fraction'] - 0.0595) < 5e-5 and abs(pm['negative_fraction'] - 0.0048) < 5e-5
    assert abs(ew['pair_violation'].max() - 0.199) < 5e-4 and abs(pm['pair_violation'].max() - 0.0146) < 5e-5
    assert pm['negative_fraction'] < ew['negative_fraction']                # Poorman improves positivity on these data
    # clipping adds exactly the negative weight
    for r in (ew, pm):
        assert abs(r['trace_weight_psd'] - r['trace_weight'] - r['negative_weight']) < 1e-14
    c = np.load(os.path.join(GOLD, 'complex_elementwise.npz'))
    h = R.positivity_ref(c['herm1_A_out'], omega=c['omega'])
    assert h['n_negative'] == 50 and abs(h['min_eigenvalue'].min() + 0.165) < 5e-4


def test_the_mirror_itself():
    for m in (1, 2, 5):
        for cplx in (False, True):
            for name, X in R.families(m, cplx, 3).items():
                r = R.hermitian_eig_ref(X)
                res, orth = R.residuals(r['H'], r['lam'], r['vec'])
                assert res.max() <= R.gate(m) and orth.max() <= R.gate(m), (m, cplx, name)
                # the projection is the nearest: its distance is out_dist, and it is positive
                assert np.allclose(R.fro(r['proj'] - r['H']), r['dist'], atol=R.gate(m) * (1 + r['fro'].max()))
                assert np.linalg.eigvalsh(r['proj']).min() >= -2 * R.gate(m) * (1 + r['fro'].max())
    assert R.gate(64) == 4 * 64 * 2.0 ** -52 and R.gate(2) == 4 * 8 * 2.0 ** -52 and R.gate(5, 1e-14) == 4e-14
    assert positivity.accuracy_gate(3) == R.gate(3) and positivity.accuracy_gate(64) == R.gate(64)
