"""What the context-free entry points refuse before they look for a device: raw ctypes calls with one bad argument each.

Every row names an entry, what is wrong with the call, and the code the library returned for it when the table was
recorded (on the commit before the entries moved onto the staging helper of maxent_amd/csrc/mxe_stage.h).  A call
that passes its checks goes on to the device -- MXE_ERR_NODEVICE where there is none --, so only refusals are in the
table, and the test runs the same with and without a GPU.  The output arrays are filled with a sentinel before the
call and must still hold it after a refusal.
"""
import ctypes

import numpy as np
import pytest

from maxent_amd import device

ARG, LIMIT, NUMERIC = -1, -5, -6
SENT = -777.25
ISENT = -777
NAN, INF = float('nan'), float('inf')
BIG = 1 << 30

NS, NB, ND, NW = 2, 5, 7, 5            # sets, bins, data points, omega points
M, N = 6, 5                            # rows and columns of a kernel matrix


def _rng():
    return np.random.default_rng(20240607)


def _outs(**shapes):
    """output arrays: float64 unless the name is in the integer list below"""
    ints = ('out_ns', 'out_info', 'out_rank', 'out_sweeps', 'out_levels')
    out = {}
    for k, n in shapes.items():
        out[k] = np.full(n, ISENT, dtype=np.int32) if k in ints else np.full(n, SENT, dtype=np.float64)
    out['out_ms'] = np.full(1, SENT, dtype=np.float32)
    return out


def _svd(grid, extra, n_grid=None):
    """the arguments the six kernel entries share, around what each has of its own (``extra``, in order after delta);
    n_grid: the rows, where the grid holds more than one value per row (the matrix of mxe_kernel_svd_data)"""
    a = dict(device=0, n_grid=len(grid) if n_grid is None else n_grid, n_omega=N, grid=grid,
             omega=np.linspace(-2.0, 2.0, N), delta=np.full(N, 1.0))
    a.update(extra)
    a.update(n_b=1, preblur_b=np.zeros(1), threshold=1e-10, ns_max=N)
    a.update(_outs(out_K=2 * M * N, out_U=2 * M * N, out_S=N, out_V=N * N, out_ns=1, out_info=3))
    return a


def _bins():
    return _rng().normal(size=(NS, NB, ND))


def _T():
    return np.tile(np.eye(ND), (NS, 1, 1))


VALID = {
    'mxe_kernel_svd': lambda: _svd(np.linspace(0.0, 2.0, M), dict(beta=2.0)),
    'mxe_kernel_svd_iw': lambda: _svd(np.pi * (2 * np.arange(M) + 1) / 2.0, {}),
    'mxe_kernel_svd_boson': lambda: _svd(np.linspace(0.0, 2.0, M), dict(beta=2.0, symmetric=0)),
    'mxe_kernel_svd_boson_iw': lambda: _svd(np.pi * 2 * np.arange(M) / 2.0, dict(symmetric=0)),
    'mxe_kernel_svd_legendre': lambda: _svd(np.arange(M, dtype=np.float64), dict(beta=2.0)),
    'mxe_kernel_svd_data': lambda: _svd(_rng().normal(size=M * N), {}, n_grid=M),      # a 6 x 5 matrix
    'mxe_kramers_kronig': lambda: dict(
        device=0, n_w=N, w=np.linspace(-2.0, 2.0, N), weight=np.full(N, 1.0), eta=np.full(N, 0.1), n_out=3,
        w_out=np.linspace(-1.0, 1.0, 3), n_spec=2, A=np.full((2, N), 0.2), **_outs(out_G=2 * 2 * 3)),
    'mxe_bins_eig': lambda: dict(
        device=0, n_sets=NS, n_bins=NB, n_data=ND, bins=_bins(), threshold=1e-12,
        **{k: v for k, v in _outs(out_mean=NS * ND, out_var=NS * ND, out_T=NS * ND * ND, out_rank=NS,
                                  out_sweeps=NS).items() if k != 'out_ms'}),
    'mxe_bins_resample': lambda: dict(
        device=0, n_sets=NS, n_bins=NB, n_data=ND, bins=_bins(), n_res=3, counts=np.ones((3, NB), dtype=np.int32), T=_T(),
        rank=np.full(NS, ND, dtype=np.int32), **_outs(out_mean=NS * ND, out_G=NS * 3 * ND, out_dev=NS * 3 * ND)),
    'mxe_bins_check': lambda: dict(
        device=0, n_sets=NS, n_bins=NB, n_data=ND, bins=_bins(), T=_T(), rank=np.full(NS, ND, dtype=np.int32),
        **_outs(out_mean=NS * ND, out_err2=NS * 2 * ND, out_skew=NS * 2 * ND, out_kurt=NS * 2 * ND, out_levels=1)),
    'mxe_mock_data': lambda: dict(
        device=0, n_sets=NS, n_mock=3, n_data=ND, n_omega=NW, K=_rng().normal(size=(ND, NW)), H0=np.full((NS, NW), 0.2),
        err=np.full((NS, ND), 0.01), T=_T(), rank=np.full(NS, ND, dtype=np.int32), seed=7,
        stream=np.arange(NS, dtype=np.uint64), **_outs(out_model=NS * ND, out_G=NS * 3 * ND)),
    'mxe_hermitian_eig': lambda: dict(
        device=0, n_mat=2, m=3, is_complex=0, A=_rng().normal(size=(2, 3, 3)), floor=0.0,
        **_outs(out_lambda=6, out_vec=18, out_proj=18, out_neg=2, out_dist=2, out_pair=2, out_asym=2, out_info=2)),
    'mxe_normals': lambda: dict(device=0, seed=1, stream=2, n_samples=3, n=4,
                                out_z=np.full(12, SENT, dtype=np.float64)),
    'mxe_entropy': lambda: dict(
        device=0, kind=0, n_omega=NW, P=2, H=np.full((2, NW), 0.2), D=np.full(NW, 0.2),
        out_S=np.full(2, SENT), out_dS=np.full(2 * NW, SENT), out_ddS=np.full(2 * NW, SENT)),
}


class Poke:
    """one element of a valid input array replaced"""
    def __init__(self, index, value):
        self.index, self.value = index, value


def _common_svd_rows(name):
    rows = [(name, 'n_grid = 0', dict(n_grid=0), ARG), (name, 'n_omega = 0', dict(n_omega=0), ARG),
            (name, 'n_b = 0', dict(n_b=0), ARG), (name, 'ns_max = 0', dict(ns_max=0), ARG),
            (name, 'ns_max = 129', dict(ns_max=129), ARG), (name, 'threshold < 0', dict(threshold=-1e-3), ARG),
            (name, 'threshold NaN', dict(threshold=NAN), ARG)]
    rows += [(name, k + ' NULL', {k: None}, ARG)
             for k in ('grid', 'omega', 'delta', 'preblur_b', 'out_U', 'out_S', 'out_V', 'out_ns')]
    return rows


# (entry, what is wrong, the arguments that differ from the valid call, the code recorded from the parent commit)
ROWS = []
for _name in ('mxe_kernel_svd', 'mxe_kernel_svd_iw', 'mxe_kernel_svd_boson', 'mxe_kernel_svd_boson_iw',
              'mxe_kernel_svd_legendre', 'mxe_kernel_svd_data'):
    ROWS += _common_svd_rows(_name)
ROWS += [
    # (8 000 rows of mxe_kernel_svd are refused too, but behind the device pick: no row here)
    ('mxe_kernel_svd_iw', 'n_iw n_omega past 2^29', dict(n_grid=1 << 28), ARG),
    ('mxe_kernel_svd_boson', 'beta = 0', dict(beta=0.0), ARG),
    ('mxe_kernel_svd_boson', 'beta NaN', dict(beta=NAN), ARG),
    ('mxe_kernel_svd_boson', 'n_tau n_omega past 2^30', dict(n_grid=1 << 29), ARG),
    ('mxe_kernel_svd_boson', 'symmetric with a negative omega', dict(symmetric=1), ARG),
    ('mxe_kernel_svd_boson', 'symmetric with a NaN omega', dict(symmetric=1, omega=np.array([0.0, 0.5, NAN, 1.5, 2.0])), ARG),
    ('mxe_kernel_svd_boson_iw', 'n_inu n_omega past 2^29', dict(n_grid=1 << 28), ARG),
    ('mxe_kernel_svd_boson_iw', 'symmetric with a negative omega', dict(symmetric=1), ARG),
    ('mxe_kernel_svd_legendre', 'beta = 0', dict(beta=0.0), ARG),
    ('mxe_kernel_svd_legendre', 'beta Inf', dict(beta=INF), ARG),
    ('mxe_kernel_svd_legendre', 'n_l n_omega past 2^29', dict(n_grid=1 << 28), ARG),
    ('mxe_kernel_svd_legendre', 'an order twice', dict(grid=Poke(3, 1.0)), ARG),
    ('mxe_kernel_svd_legendre', 'an order that is no integer', dict(grid=Poke(2, 2.5)), ARG),
    ('mxe_kernel_svd_legendre', 'a negative order', dict(grid=Poke(0, -1.0)), ARG),
    ('mxe_kernel_svd_legendre', 'an order NaN', dict(grid=Poke(5, NAN)), ARG),
    ('mxe_kernel_svd_legendre', 'an order beyond the largest', dict(grid=Poke(5, 1.0e6)), ARG),
    ('mxe_kernel_svd_legendre', 'beta |omega| / 2 too large', dict(omega=Poke(0, -1.0e9)), ARG),
    ('mxe_kernel_svd_legendre', 'omega NaN', dict(omega=Poke(4, NAN)), ARG),
    ('mxe_kernel_svd_data', 'NaN in the matrix', dict(grid=Poke(M * N - 1, NAN)), NUMERIC),
    ('mxe_kernel_svd_data', 'Inf in the matrix', dict(grid=Poke(0, INF)), NUMERIC),
    ('mxe_kernel_svd_data', '8 000 rows', dict(n_grid=8000, grid=np.zeros(8000 * N)), LIMIT),
    ('mxe_kernel_svd_data', 'n_rows n_omega past 2^30', dict(n_grid=1 << 29), ARG),

    ('mxe_kramers_kronig', 'n_w = 0', dict(n_w=0), ARG),
    ('mxe_kramers_kronig', 'n_out = 0', dict(n_out=0), ARG),
    ('mxe_kramers_kronig', 'n_spec = 0', dict(n_spec=0), ARG),
    ('mxe_kramers_kronig', 'n_spec n_out past 2^31 - 1', dict(n_spec=70000, n_out=70000), ARG),
    ('mxe_kramers_kronig', 'n_spec n_w past 2^31 - 1', dict(n_spec=70000, n_w=70000), ARG),
] + [('mxe_kramers_kronig', k + ' NULL', {k: None}, ARG) for k in ('w', 'weight', 'eta', 'w_out', 'A', 'out_G')] + [

    ('mxe_bins_eig', 'n_sets = 0', dict(n_sets=0), ARG),
    ('mxe_bins_eig', 'n_bins = 1', dict(n_bins=1), ARG),
    ('mxe_bins_eig', 'n_data = 0', dict(n_data=0), ARG),
    ('mxe_bins_eig', 'n_data = 513', dict(n_data=513), ARG),
    ('mxe_bins_eig', 'threshold < 0', dict(threshold=-1.0), ARG),
    ('mxe_bins_eig', 'threshold NaN', dict(threshold=NAN), ARG),
    ('mxe_bins_eig', 'threshold Inf', dict(threshold=INF), ARG),
    ('mxe_bins_eig', 'n_bins n_data past 2^31 - 1', dict(n_bins=1 << 23, n_data=512), ARG),
    ('mxe_bins_eig', 'NaN in the last bin value', dict(bins=Poke(NS * NB * ND - 1, NAN)), ARG),
    ('mxe_bins_eig', 'Inf in the first bin value', dict(bins=Poke(0, INF)), ARG),
] + [('mxe_bins_eig', k + ' NULL', {k: None}, ARG)
     for k in ('bins', 'out_mean', 'out_var', 'out_T', 'out_rank', 'out_sweeps')] + [

    ('mxe_bins_resample', 'n_sets = 0', dict(n_sets=0), ARG),
    ('mxe_bins_resample', 'n_bins = 1', dict(n_bins=1), ARG),
    ('mxe_bins_resample', 'n_data = 513', dict(n_data=513), ARG),
    ('mxe_bins_resample', 'n_res = 0', dict(n_res=0), ARG),
    ('mxe_bins_resample', 'n_res n_bins past 2^31 - 1', dict(n_res=BIG), ARG),
    ('mxe_bins_resample', 'a negative count', dict(counts=Poke(4, -1)), ARG),
    ('mxe_bins_resample', 'a resample without bins', dict(counts=np.zeros((3, NB), dtype=np.int32)), ARG),
    ('mxe_bins_resample', 'a negative rank', dict(rank=Poke(1, -1)), ARG),
    ('mxe_bins_resample', 'a rank above n_data', dict(rank=Poke(0, ND + 1)), ARG),
    ('mxe_bins_resample', 'NaN in bins', dict(bins=Poke(NS * NB * ND - 1, NAN)), ARG),
    ('mxe_bins_resample', 'Inf in T', dict(T=Poke(NS * ND * ND - 1, INF)), ARG),
] + [('mxe_bins_resample', k + ' NULL', {k: None}, ARG) for k in ('bins', 'counts', 'T', 'rank', 'out_mean', 'out_G')] + [

    ('mxe_bins_check', 'n_sets = 0', dict(n_sets=0), ARG),
    ('mxe_bins_check', 'n_bins = 1', dict(n_bins=1), ARG),
    ('mxe_bins_check', 'n_data = 513', dict(n_data=513), ARG),
    ('mxe_bins_check', 'n_bins n_data past 2^31 - 1', dict(n_bins=1 << 23, n_data=512), ARG),
    ('mxe_bins_check', 'T without rank', dict(rank=None), ARG),
    ('mxe_bins_check', 'rank without T', dict(T=None), ARG),
    ('mxe_bins_check', 'a negative rank', dict(rank=Poke(0, -1)), ARG),
    ('mxe_bins_check', 'NaN in bins', dict(bins=Poke(NS * NB * ND - 1, NAN)), ARG),
    ('mxe_bins_check', 'NaN in T', dict(T=Poke(3, NAN)), ARG),
] + [('mxe_bins_check', k + ' NULL', {k: None}, ARG)
     for k in ('bins', 'out_mean', 'out_err2', 'out_skew', 'out_kurt', 'out_levels')] + [

    ('mxe_mock_data', 'n_sets = 0', dict(n_sets=0), ARG),
    ('mxe_mock_data', 'n_mock = 0', dict(n_mock=0), ARG),
    ('mxe_mock_data', 'n_data = 0', dict(n_data=0), ARG),
    ('mxe_mock_data', 'n_omega = 0', dict(n_omega=0), ARG),
    ('mxe_mock_data', 'T without rank', dict(rank=None), ARG),
    ('mxe_mock_data', 'rank without T', dict(T=None), ARG),
    ('mxe_mock_data', 'n_sets n_mock n_data past 2^31 - 1', dict(n_mock=BIG), ARG),
    ('mxe_mock_data', 'NaN in K', dict(K=Poke(ND * NW - 1, NAN)), ARG),
    ('mxe_mock_data', 'Inf in H0', dict(H0=Poke(NS * NW - 1, INF)), ARG),
    ('mxe_mock_data', 'NaN in err', dict(err=Poke(NS * ND - 1, NAN)), ARG),
    ('mxe_mock_data', 'err = 0', dict(err=Poke(2, 0.0)), ARG),
    ('mxe_mock_data', 'err < 0', dict(err=Poke(2, -0.01)), ARG),
    ('mxe_mock_data', 'a negative rank', dict(rank=Poke(1, -1)), ARG),
    ('mxe_mock_data', 'a rank above n_data', dict(rank=Poke(1, ND + 1)), ARG),
    ('mxe_mock_data', 'NaN in T', dict(T=Poke(NS * ND * ND - 1, NAN)), ARG),
] + [('mxe_mock_data', k + ' NULL', {k: None}, ARG) for k in ('K', 'H0', 'err', 'stream', 'out_model', 'out_G')] + [

    ('mxe_hermitian_eig', 'n_mat = 0', dict(n_mat=0), ARG),
    ('mxe_hermitian_eig', 'm = 0', dict(m=0), ARG),
    ('mxe_hermitian_eig', 'm = 65', dict(m=65), LIMIT),
    ('mxe_hermitian_eig', 'is_complex = 2', dict(is_complex=2), ARG),
    ('mxe_hermitian_eig', 'A NULL', dict(A=None), ARG),
    ('mxe_hermitian_eig', 'floor NaN', dict(floor=NAN), ARG),
    ('mxe_hermitian_eig', 'floor Inf', dict(floor=INF), ARG),
    ('mxe_hermitian_eig', 'n_mat m m past 2^31 - 1', dict(n_mat=1 << 20, m=64), ARG),

    ('mxe_normals', 'n_samples = 0', dict(n_samples=0), ARG),
    ('mxe_normals', 'n = 0', dict(n=0), ARG),
    ('mxe_normals', 'out_z NULL', dict(out_z=None), ARG),
    ('mxe_normals', 'n_samples n past 2^31 - 1', dict(n_samples=70000, n=70000), ARG),

    ('mxe_entropy', 'n_omega = 0', dict(n_omega=0), ARG),
    ('mxe_entropy', 'P = 0', dict(P=0), ARG),
    ('mxe_entropy', 'H NULL', dict(H=None), ARG),
    ('mxe_entropy', 'D NULL', dict(D=None), ARG),
    ('mxe_entropy', 'kind = 2', dict(kind=2), ARG),
    ('mxe_entropy', 'kind = -1', dict(kind=-1), ARG),
]


def call(lib, name, changes):
    """the valid call of ``name`` with ``changes`` applied; returns (code, the output arrays that were handed in)"""
    args = VALID[name]()
    for k, v in changes.items():
        assert k in args, (name, k)
        if isinstance(v, Poke):
            a = np.array(args[k], copy=True)
            a.reshape(-1)[v.index] = v.value
            v = a
        args[k] = v
    fn = getattr(lib, name)
    assert len(fn.argtypes) == len(args), (name, len(fn.argtypes), len(args))
    keep, cargs = [], []
    for (k, v), t in zip(args.items(), fn.argtypes):
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            assert ctypes.sizeof(t._type_) == v.dtype.itemsize, (name, k, v.dtype)
            keep.append((k, v))
            cargs.append(v.ctypes.data_as(t))
        else:
            cargs.append(v)
    rc = fn(*cargs)
    return rc, {k: v for k, v in keep if k.startswith('out_')}


@pytest.fixture(scope='module')
def lib():
    return device.load_library()


def test_every_context_free_entry_has_rows():
    assert {r[0] for r in ROWS} == set(VALID) and len(VALID) == 14


@pytest.mark.parametrize('name,what,changes,code', ROWS, ids=['%s: %s' % (r[0][4:], r[1]) for r in ROWS])
def test_refusal(lib, name, what, changes, code):
    rc, outs = call(lib, name, changes)
    assert rc == code, '%s with %s returned %d (%s)' % (name, what, rc, lib.mxe_strerror(rc).decode())
    for k, a in outs.items():
        sent = ISENT if a.dtype == np.int32 else SENT
        assert np.all(a == sent), '%s with %s wrote to %s' % (name, what, k)
