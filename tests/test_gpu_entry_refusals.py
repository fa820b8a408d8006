"""What the context-bound single-launch entry points refuse: raw ctypes calls with one bad argument each, on one small
context (40 x 64, two elements, ten alphas, one launch).

Every row names an entry, what is wrong with the call, and the code the library returned for it when the table was
recorded (on the commit before the entries moved onto the staging helper of maxent_amd/csrc/mxe_stage.h).  Every row is
an argument error that returns before any launch; the output arrays are filled with a sentinel before the call and must
still hold it afterwards.  After the table one valid call of every entry returns MXE_OK: a refusal leaves the context
usable.
"""
import ctypes

import numpy as np
import pytest

from maxent_amd import device, synthetic, hostprep

pytestmark = pytest.mark.gpu

OK, ARG, STATE, LIMIT = 0, -1, -4, -5
SENT, ISENT = -777.25, -777
NAN, INF = float('nan'), float('inf')
P, NW, NA, NT = 4, 64, 10, 40          # problems of a call, omega points, alphas of the launch, rows of the data set


def f(n):
    return np.full(n, SENT, dtype=np.float64)


def i(n):
    return np.full(n, ISENT, dtype=np.int32)


def ms():
    return np.full(1, SENT, dtype=np.float32)


class Job(object):
    def __init__(self, launch):
        tau, omega, K, G = synthetic.single_G(NT, NW)
        K.reduce_singular_space(1e-14)
        D = synthetic.flat_D(omega)
        err = synthetic.SIGMA * (1.0 + np.random.RandomState(1).rand(NT))
        self.alphas = np.array(synthetic.alpha_mesh(NA)) * NT
        self.n_s = len(K.S)
        self.ctx = device.DeviceContext(K.U, K.S, K.V)
        ds = self.ctx.add_dataset(err)
        kinds = [device.ENTROPY_NORMAL, device.ENTROPY_PLUSMINUS]
        self.ctx.set_elements([ds] * 2, [G, G], np.tile(D, (2, 1)), kinds)
        if launch:
            v0 = np.stack([hostprep.initial_v(K.V, D, omega.delta, k) for k in kinds])
            sol = self.ctx.solve_chains(np.arange(2), self.alphas, v0)
            assert sol['converged'].all()


@pytest.fixture(scope='module')
def jobs():
    js = {'launched': Job(True), 'fresh': Job(False)}
    yield js
    for j in js.values():
        j.ctx.close()


def _post(al):
    return dict(P=P, elem=np.zeros(P, dtype=np.int32), alpha=np.array(al[:P]), H=None,
                problem_index=np.arange(P, dtype=np.int32), chi2_factor=1.0)


def _groups():
    return dict(n_groups=2, group_offset=np.array([0, 2, 4], dtype=np.int32), H=None,
                problem_index=np.arange(4, dtype=np.int32))


VALID = {
    'mxe_posterior_var': lambda j: dict(_post(j.alphas), n_f=2, F=np.full((2, NW), 0.5), out_var=f(P * 2), out_diag=f(P * NW),
                                         out_prior=f(P * 2), out_ms=ms()),
    'mxe_posterior_sample': lambda j: dict(_post(j.alphas), n_samples=2, seed=5, stream=None, z=np.full((P, 2, NW + j.n_s), 0.25),
                                            out_dH=f(P * 2 * NW), out_ms=ms()),
    'mxe_fit_diagnostics': lambda j: dict(_post(j.alphas), ld=NT, out_ngood=f(P), out_chi2=f(P), out_resid=f(P * NT),
                                           out_lev=f(P * NT), out_ms=ms()),
    'mxe_response': lambda j: dict(_post(j.alphas), space=0, weighted=1, n_rhs=2, ld=NW, F=np.full((P, 2, NW), 0.5),
                                    out_X=f(P * 2 * NW), out_ms=ms()),
    'mxe_resample_reduce': lambda j: dict(_groups(), scale=np.ones(2), n_f=1, F=np.full((1, NW), 0.5), out_mean=f(2 * NW),
                                           out_var=f(2 * NW), out_fval=f(4), out_fmean=f(2), out_fcov=f(2), out_used=i(2),
                                           out_ms=ms()),
    'mxe_resample_quantiles': lambda j: dict(_groups(), n_q=2, q=np.array([0.25, 0.75]), out_q=f(2 * 2 * NW), out_used=i(2),
                                              out_ms=ms()),
    'mxe_evidence_reduce': lambda j: dict(
        n_groups=1, group_offset=np.array([0, 2], dtype=np.int32), n_alpha=NA, H=None, chain_index=None,
        logp=np.linspace(-3.0, -1.0, 2 * NA), log_quad=np.zeros(NA), log_mix=np.zeros(NA), log_prior=None, row_mode=0,
        pick=np.zeros(2, dtype=np.int32), n_f=1, F=np.full((1, NW), 0.5), out_logZ=f(2), out_kmax=i(2), out_ngood=i(2),
        out_walpha=f(2 * NA), out_row=f(2 * NW), out_fval=f(2), out_wmodel=f(2), out_mean=f(NW), out_between=f(NW),
        out_fmean=f(1), out_fcov=f(1), out_used=i(1), out_ms=ms()),
}
POSTERIOR = ('mxe_posterior_var', 'mxe_posterior_sample', 'mxe_fit_diagnostics', 'mxe_response')
GROUPED = ('mxe_resample_reduce', 'mxe_resample_quantiles')


class Poke:
    """one element of a valid input array replaced"""
    def __init__(self, index, value):
        self.index, self.value = index, value


# (entry, what is wrong, the arguments that differ from the valid call, the code recorded from the parent commit);
# a fifth entry 'fresh': the call goes to the context that has not launched
ROWS = []
for _n in POSTERIOR:
    ROWS += [(_n, 'P = 0', dict(P=0), ARG), (_n, 'elem NULL', dict(elem=None), ARG), (_n, 'alpha NULL', dict(alpha=None), ARG),
             (_n, 'alpha = 0', dict(alpha=Poke(1, 0.0)), ARG), (_n, 'alpha < 0', dict(alpha=Poke(3, -1.0)), ARG),
             (_n, 'alpha NaN', dict(alpha=Poke(0, NAN)), ARG), (_n, 'chi2_factor = 0', dict(chi2_factor=0.0), ARG),
             (_n, 'chi2_factor Inf', dict(chi2_factor=INF), ARG), (_n, 'an element past the last', dict(elem=Poke(2, 2)), ARG),
             (_n, 'a negative element', dict(elem=Poke(0, -1)), ARG),
             (_n, 'a row past the launch', dict(problem_index=Poke(3, 2 * NA)), ARG),
             (_n, 'a negative row', dict(problem_index=Poke(0, -1)), ARG),
             (_n, 'H NULL before any launch', {}, STATE, 'fresh')]
for _n in GROUPED:
    ROWS += [(_n, 'n_groups = 0', dict(n_groups=0), ARG), (_n, 'group_offset NULL', dict(group_offset=None), ARG),
             (_n, 'group_offset[0] = 1', dict(group_offset=Poke(0, 1)), ARG),
             (_n, 'offsets that decrease', dict(group_offset=np.array([0, 3, 2], dtype=np.int32)), ARG),
             (_n, 'a row past the launch', dict(problem_index=Poke(1, 2 * NA)), ARG),
             (_n, 'a row past the launch, no index', dict(group_offset=np.array([0, 2, 2 * NA + 1], dtype=np.int32),
                                                         problem_index=None), ARG),
             (_n, 'H NULL before any launch', {}, STATE, 'fresh')]
ROWS += [
    ('mxe_posterior_var', 'n_f < 0', dict(n_f=-1), ARG),
    ('mxe_posterior_var', 'F NULL', dict(F=None), ARG),
    ('mxe_posterior_var', 'out_var NULL', dict(out_var=None), ARG),
    ('mxe_posterior_var', 'neither F nor out_diag', dict(n_f=0, F=None, out_var=None, out_prior=None, out_diag=None), ARG),
    ('mxe_posterior_var', 'out_prior without F', dict(n_f=0, F=None, out_var=None), ARG),
    ('mxe_posterior_var', 'NaN in F', dict(F=Poke(2 * NW - 1, NAN)), ARG),
    ('mxe_posterior_sample', 'n_samples = 0', dict(n_samples=0), ARG),
    ('mxe_posterior_sample', 'out_dH NULL', dict(out_dH=None), ARG),
    ('mxe_posterior_sample', 'neither z nor stream', dict(z=None), ARG),
    ('mxe_posterior_sample', 'NaN in z', dict(z=Poke(-1, NAN)), ARG),
    ('mxe_fit_diagnostics', 'ld = 0', dict(ld=0), ARG),
    ('mxe_fit_diagnostics', 'ld below the rows of the data set', dict(ld=NT - 1), ARG),
    ('mxe_response', 'F NULL', dict(F=None), ARG),
    ('mxe_response', 'out_X NULL', dict(out_X=None), ARG),
    ('mxe_response', 'n_rhs = 0', dict(n_rhs=0), ARG),
    ('mxe_response', 'space = 2', dict(space=2), ARG),
    ('mxe_response', 'model space: ld below n_omega', dict(ld=NW - 1), ARG),
    ('mxe_response', 'data space: ld below the rows of the data set', dict(space=1, ld=NT - 1), ARG),
    ('mxe_response', 'Inf in F', dict(F=Poke(P * 2 * NW - 1, INF)), ARG),
    ('mxe_response', 'P n_rhs n_omega past 2^31 - 1', dict(n_rhs=1 << 23), ARG),
    ('mxe_resample_reduce', 'scale NULL', dict(scale=None), ARG),
    ('mxe_resample_reduce', 'scale NaN', dict(scale=Poke(1, NAN)), ARG),
    ('mxe_resample_reduce', 'n_f < 0', dict(n_f=-1), ARG),
    ('mxe_resample_reduce', 'F NULL', dict(F=None), ARG),
    ('mxe_resample_reduce', 'NaN in F', dict(F=Poke(NW - 1, NAN)), ARG),
    ('mxe_resample_quantiles', 'n_q = 0', dict(n_q=0), ARG),
    ('mxe_resample_quantiles', 'q NULL', dict(q=None), ARG),
    ('mxe_resample_quantiles', 'q above 1', dict(q=Poke(1, 1.5)), ARG),
    ('mxe_resample_quantiles', 'q below 0', dict(q=Poke(0, -0.1)), ARG),
    ('mxe_resample_quantiles', 'q NaN', dict(q=Poke(0, NAN)), ARG),
    ('mxe_resample_quantiles', 'a group of MXE_QUANTILE_MAX_ROWS + 1 rows',
     dict(n_groups=1, group_offset=np.array([0, device.QUANTILE_MAX_ROWS + 1], dtype=np.int32),
          H=np.full((device.QUANTILE_MAX_ROWS + 1, NW), 0.5), problem_index=None), LIMIT),
    ('mxe_evidence_reduce', 'n_groups = 0', dict(n_groups=0), ARG),
    ('mxe_evidence_reduce', 'group_offset NULL', dict(group_offset=None), ARG),
    ('mxe_evidence_reduce', 'group_offset[0] = 1', dict(group_offset=Poke(0, 1)), ARG),
    ('mxe_evidence_reduce', 'offsets that decrease', dict(n_groups=2, group_offset=np.array([0, 2, 1], dtype=np.int32)), ARG),
    ('mxe_evidence_reduce', 'n_alpha = 0', dict(n_alpha=0), ARG),
    ('mxe_evidence_reduce', 'n_alpha that is not the launch\'s', dict(n_alpha=NA - 1), ARG),
    ('mxe_evidence_reduce', 'logp NULL', dict(logp=None), ARG),
    ('mxe_evidence_reduce', 'log_quad NULL', dict(log_quad=None), ARG),
    ('mxe_evidence_reduce', 'log_mix NULL', dict(log_mix=None), ARG),
    ('mxe_evidence_reduce', 'F NULL', dict(F=None), ARG),
    ('mxe_evidence_reduce', 'row_mode = 3', dict(row_mode=3), ARG),
    ('mxe_evidence_reduce', 'row_mode = -1', dict(row_mode=-1), ARG),
    ('mxe_evidence_reduce', 'row_mode = 2 without pick', dict(row_mode=2, pick=None), ARG),
    ('mxe_evidence_reduce', 'pick = n_alpha', dict(row_mode=2, pick=Poke(1, NA)), ARG),
    ('mxe_evidence_reduce', 'a scan past the launch', dict(chain_index=np.array([0, 2], dtype=np.int32)), ARG),
    ('mxe_evidence_reduce', 'a negative scan', dict(chain_index=np.array([-1, 1], dtype=np.int32)), ARG),
    ('mxe_evidence_reduce', 'NaN in log_quad', dict(log_quad=Poke(NA - 1, NAN)), ARG),
    ('mxe_evidence_reduce', 'Inf in log_mix', dict(log_mix=Poke(0, INF)), ARG),
    ('mxe_evidence_reduce', 'NaN in F', dict(F=Poke(NW - 1, NAN)), ARG),
    ('mxe_evidence_reduce', 'log_prior NaN', dict(log_prior=np.array([0.0, NAN])), ARG),
    ('mxe_evidence_reduce', 'log_prior +Inf', dict(log_prior=np.array([INF, 0.0])), ARG),
    ('mxe_evidence_reduce', 'H NULL before any launch', {}, STATE, 'fresh'),
]


def call(job, name, changes):
    """the valid call of ``name`` with ``changes`` applied; returns (code, the output arrays that were handed in)"""
    args = VALID[name](job)
    for k, v in changes.items():
        assert k in args, (name, k)
        if isinstance(v, Poke):
            a = np.array(args[k], copy=True)
            a.reshape(-1)[v.index] = v.value
            v = a
        args[k] = v
    fn = getattr(job.ctx._lib, name)
    assert len(fn.argtypes) == len(args) + 1, (name, len(fn.argtypes), len(args))
    keep, cargs = [], [job.ctx._h]
    for (k, v), t in zip(args.items(), fn.argtypes[1:]):
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            assert ctypes.sizeof(t._type_) == v.dtype.itemsize, (name, k, v.dtype)
            keep.append((k, v))
            cargs.append(v.ctypes.data_as(t))
        else:
            cargs.append(v)
    rc = fn(*cargs)
    return rc, {k: v for k, v in keep if k.startswith('out_')}


def test_refusals_then_valid_calls(jobs):
    assert {r[0] for r in ROWS} == set(VALID) and len(VALID) == 7
    wrong = []
    for row in ROWS:
        name, what, changes, code = row[:4]
        job = jobs[row[4] if len(row) > 4 else 'launched']
        rc, outs = call(job, name, changes)
        print('%-24s %-50s %d' % (name[4:], what, rc))
        if rc != code:
            wrong.append((name, what, rc, code))
        for k, a in outs.items():
            if not np.all(a == (ISENT if a.dtype == np.int32 else SENT)):
                wrong.append((name, what, 'wrote to ' + k))
    assert not wrong, wrong
    # the context is as usable as before: one valid call of every entry
    for name in VALID:
        rc, outs = call(jobs['launched'], name, {})
        assert rc == OK, (name, rc, jobs['launched'].ctx._lib.mxe_last_hip_error(jobs['launched'].ctx._h))
        for k, a in outs.items():
            if k != 'out_prior':
                assert not np.any(a == (ISENT if a.dtype == np.int32 else SENT)), (name, k)
