"""``eval_kernel`` (through ``mxe_eval_batch`` and ``mxe_audit``) and ``entropy_kernel`` against extended precision.

The reference, its scales, the a-priori gate lengths and the synthetic problems are those of tests/eval_ref.py;
tests/test_eval_ref_host.py shows without a GPU that the reference reproduces the reference project's fixtures and that
these gates catch ten seeded faults of the kernel's arithmetic.  Here the device has to pass them:

* every one of the eleven outputs, entry by entry, within ``C eps scale`` -- ten shapes (both instantiations, one to
  seven trips of the 256-stride loops, the odd tail, one and several MFMA tiles, both padding rules), three data sets
  (scalar error, tau-dependent error, ``U_rot``), four elements of both entropies, seven problems per call; an
  eleventh shape, which the library refuses, is pinned as refused;
* the bytes of a problem do not depend on the batch, and an output does not depend on which others are asked for;
* the audit reports the correction that is there: ``corr`` against the exact Newton correction at the fetched ``v``,
  far from the minimiser and at it, ``gmax`` within its eps-scaled gate, rows and columns where the header says;
* ``mxe_entropy`` where its threads loop.
"""

import numpy as np
import pytest

import eval_ref as R
from eval_ref import NORMAL, PLUSMINUS, OUTPUTS, ELEM_DS, ELEM_KIND, AUDIT_R, AUDIT_F
from maxent_amd import device

pytestmark = pytest.mark.gpu

_CTX = {}


def context(shape):
    """one device context per shape: three data sets, four elements"""
    if shape not in _CTX:
        c = R.make_case(*shape)
        ctx = device.DeviceContext(c.U, c.S, c.V, device=0)
        ds = [ctx.add_dataset(c.err[d], c.U_rot_arg[d]) for d in range(3)]
        ctx.set_elements([ds[d] for d in ELEM_DS], c.G, c.D, list(ELEM_KIND))
        _CTX[shape] = ctx
    return _CTX[shape]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()


def run(shape, eta, input_is_H, want=OUTPUTS, only=None):
    c = R.make_case(*shape)
    x = c.Himg if input_is_H else c.v
    sel = slice(None) if only is None else slice(only, only + 1)
    return context(shape).eval_batch(c.elem[sel], c.alpha[sel], x[sel], input_is_H=input_is_H, chi2_factor=eta, want=want)


@pytest.mark.parametrize('shape', R.DEVICE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_every_output_entry_by_entry(shape):
    c = R.make_case(*shape)
    worst = dict((k, 0.0) for k in OUTPUTS)          # error / (eps scale)
    used = dict((k, 0.0) for k in OUTPUTS)           # ... as a fraction of the gate C of its problem
    left = []
    for eta in R.ETAS:
        for is_H in (False, True):
            dev = run(shape, eta, is_H)
            ref = R.case_reference(shape[0], shape[1], eta, is_H)
            for p in range(c.P):
                ro, rs, C = ref[p]
                for k in OUTPUTS:
                    ratio = R.worst_ratio(dev[k][p], ro[k], rs[k])
                    worst[k], used[k] = max(worst[k], ratio), max(used[k], ratio / C[k])
                    if not ratio <= C[k]:
                        left.append((k, eta, is_H, p, ratio, C[k]))
    print('TABLE %dx%d | ' % shape + ' | '.join('%s %.1f' % (k, worst[k]) for k in OUTPUTS))
    print('OF ITS GATE %dx%d | ' % shape + ' | '.join('%s %.2f' % (k, used[k]) for k in OUTPUTS))
    assert not left, left


@pytest.mark.parametrize('shape', R.DEVICE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_bits_of_a_problem_do_not_depend_on_the_batch(shape):
    """one workgroup per problem, a fixed order of summation: the same point alone and at its place in the batch"""
    c = R.make_case(*shape)
    p = c.P - 2 if c.P > 2 else 1                   # place 6 of 7
    for is_H in (False, True):
        full, alone = run(shape, 2.5, is_H), run(shape, 2.5, is_H, only=p)
        for k in OUTPUTS:
            assert full[k][p].tobytes() == alone[k][0].tobytes(), (k, is_H)


@pytest.mark.parametrize('shape', R.DEVICE_SHAPES, ids=lambda s: '%dx%d' % s)
def test_outputs_not_asked_for_are_not_required(shape):
    full = run(shape, 1.0, False)
    assert run(shape, 1.0, False, want=('W2',))['W2'].tobytes() == full['W2'].tobytes()
    assert run(shape, 1.0, False, want=('u', 'q'))['q'].tobytes() == full['q'].tobytes()


@pytest.mark.parametrize('shape', R.REFUSED_SHAPES, ids=lambda s: '%dx%d' % s)
def test_a_mesh_that_does_not_fit_beside_the_matrix_is_refused(shape):
    """n_s = 128 with 1537 frequencies (padded to 1792): w and H do not fit the 160 KB of LDS next to the 128 x 129
    matrix.  ``mxe_eval_batch`` says so (MXE_ERR_LIMIT) and writes nothing; the longest mesh NP = 128 takes, 1408, is
    among the shapes above."""
    c = R.make_case(*shape)
    ctx = context(shape)
    with pytest.raises(device.MaxEntDeviceError, match='exceeds kernel limits'):
        ctx.eval_batch(c.elem, c.alpha, c.v, want=OUTPUTS)
    with pytest.raises(device.MaxEntDeviceError, match='exceeds kernel limits'):
        ctx.eval_batch(c.elem[:1], c.alpha[:1], c.Himg[:1], input_is_H=True, want=('Q',))


# ---------------------------------------------------------------------------------------------------------------------
#  the audit
# ---------------------------------------------------------------------------------------------------------------------

def loose_opts(**kw):
    return device.default_opts(tol_h=1e-2, tol_d=0.0, tol_relq=0.0, stop_estimate=0, **kw)


def solve_and_audit(shape, elem, alpha, opts):
    c, ctx = R.make_case(*shape), context(shape)
    v0 = np.tile(R.audit_v0(c), (len(elem), 1))
    out = ctx.solve_chains(elem, alpha, v0, opts)
    a = ctx.audit()
    alpha2 = np.broadcast_to(alpha, (len(elem), np.shape(alpha)[-1]))
    cref, gref, ggate = R.audit_reference(shape[0], shape[1], elem, alpha2, out['v'])
    return a['corr'], a['gmax'], cref, gref, ggate, out['v']


@pytest.mark.parametrize('chains_per_wg', (1, 4))
@pytest.mark.parametrize('shape', R.AUDIT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_audit_reports_the_correction_that_is_there(shape, chains_per_wg):
    elem = [0, 1, 2, 3]
    for loose in (True, False):
        opts = loose_opts(chains_per_wg=chains_per_wg) if loose else device.default_opts(chains_per_wg=chains_per_wg)
        corr, gmax, cref, gref, ggate, _ = solve_and_audit(shape, elem, R.AUDIT_ALPHAS, opts)
        d = np.abs(corr - cref)
        far = cref >= 1e-6
        print('AUDIT %dx%d cpw=%d %s: problems with corr_ref in [1e-6, 1e-1]: %d of %d; worst |d| / corr_ref there %.2e; '
              'worst |d| where corr_ref < 1e-7: %.2e; max corr_ref %.2e; worst gmax error / gate %.3f' % (
                  shape[0], shape[1], chains_per_wg, 'loose' if loose else 'default',
                  np.sum(far & (cref <= 1e-1)), cref.size, np.max(d[far] / cref[far]) if far.any() else 0.0,
                  np.max(d[cref < 1e-7]) if (cref < 1e-7).any() else 0.0, cref.max(), np.max(np.abs(gmax - gref) / ggate)))
        if loose:
            assert 3 * np.sum(far & (cref <= 1e-1)) >= cref.size, ('vacuous: the loose runs do not stop far from the minimiser', cref)
        else:
            assert cref.max() < 1e-7, cref
        assert np.all(d <= AUDIT_R * cref + AUDIT_F), (corr, cref)
        assert np.all(np.abs(gmax - gref) <= ggate), (gmax, gref, ggate)


@pytest.mark.parametrize('shape', R.AUDIT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_audit_is_indexed_chain_by_alpha(shape):
    """[n_chain][n_alpha] with the element and the alpha of that chain: two chains on different elements (and data
    sets), two alpha lists of one length; no permutation of the expected matrix passes as well"""
    elem = [1, 2]
    alpha = np.array([[10.0, 1.0, 0.1], [3.0, 0.3, 0.03]])
    corr, gmax, cref, gref, ggate, v = solve_and_audit(shape, elem, alpha, loose_opts())

    def passes(expected):
        return bool(np.all(np.abs(corr - expected) <= AUDIT_R * expected + AUDIT_F))
    assert passes(cref), (corr, cref)
    others = [cref[::-1], cref[:, ::-1], cref[::-1, ::-1], cref.T.reshape(2, 3), cref.reshape(3, 2).T]
    assert not any(passes(np.ascontiguousarray(x)) for x in others), (corr, cref)
    # and with the wrong element or alpha the reference itself differs by more than the gate
    wrong_e = R.audit_reference(shape[0], shape[1], elem[::-1], alpha, v)[0]
    assert not passes(wrong_e)


# ---------------------------------------------------------------------------------------------------------------------
#  mxe_entropy
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', (NORMAL, PLUSMINUS), ids=('normal', 'plusminus'))
@pytest.mark.parametrize('n', (1, 255, 256, 257, 1000))
def test_entropy_where_the_threads_loop(n, kind):
    rng = np.random.RandomState(77 + n)
    P = 3
    D = 10.0 ** (-2 + 2 * rng.rand(n))
    H = D[None, :] * np.exp(2.0 * rng.randn(P, n))
    edges = (0.0, 1e-120) if kind == NORMAL else (1e3, -1e3, 1e-9, 0.0)      # in units of D
    if kind == PLUSMINUS:
        H *= np.sign(rng.randn(P, n))
    for p in range(P):
        for j, f in enumerate(edges):
            i = (17 * p + j) % n
            H[p, i] = f * D[i]
    S, dS, ddS = device.entropy(kind, H, D)
    o, s = R.entropy_ref(kind, H, D)
    # S: a sum of n terms, gated as (n + 8) eps sum|terms|; d and dd: 8 ulps of their scale (a logarithm of a quotient,
    # a reciprocal of a sum: a handful of roundings each)
    rS, rd, rdd = R.worst_ratio(S, o['S'], s['S']), R.worst_ratio(dS, o['d'], s['d']), R.worst_ratio(ddS, o['dd'], s['dd'])
    print('ENTROPY n=%d kind=%d: error / (eps scale): S %.2f  d %.2f  dd %.2f' % (n, kind, rS, rd, rdd))
    assert rS <= n + 8 and rd <= 8 and rdd <= 8, (rS, rd, rdd)
