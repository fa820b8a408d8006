"""The extended-precision reference of the cost-function kernels (tests/eval_ref.py) and its gates, without a GPU.

1. The reference reproduces the numbers of the reference project: every ``n_* / pm_* / b_*`` entry of
   ``tests/golden/derivs.npz`` through the combinations of ``cost_functions.py``, and ``plusminus_entropy.npz``.
2. The gates bite: a binary64 numpy restatement of the arithmetic of ``eval_kernel`` and of the host part of
   ``mxe_eval_batch`` / ``mxe_audit`` (:class:`Model`) passes every gate of tests/test_gpu_eval_truth.py at every
   shape, and leaves at least one gate with each of ten seeded faults, at every shape where the fault can act.
3. The audit cases are not vacuous: the loose solves stop where the true correction is between 1e-6 and 1e-1, the
   default solves below 1e-7 (the oracle's ``alpha_chain`` stands in for the chain kernel here).
"""

import functools
import os

import numpy as np
import pytest

import eval_ref as R
from eval_ref import LD, NORMAL, PLUSMINUS, OUTPUTS, ELEM_DS, ELEM_KIND
from oracle import sform

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# the gate of the audit's corr, |corr - corr_ref| <= AUDIT_R corr_ref + AUDIT_F: 8 x the worst seen on the device
# ("The checker, checked"); tests/test_gpu_eval_truth.py asserts the same two numbers
AUDIT_R, AUDIT_F = R.AUDIT_R, R.AUDIT_F


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b ** 2)))


# ---------------------------------------------------------------------------------------------------------------------
#  1. the fixtures of the reference project
# ---------------------------------------------------------------------------------------------------------------------

def test_reference_reproduces_every_derivative_fixture():
    z = np.load(os.path.join(GOLD, 'derivs.npz'))
    b = R.RefBasis(z['U'], z['S'], z['V'], z['err'])
    alpha, V, M = float(z['alpha']), b.V, b.M()
    TOL = 1e-11
    worst = {}

    def check(name, got):
        e = rel(got, z[name])
        worst[name] = e
        assert e < TOL, (name, e)

    def modes(o, eta):
        W, g, W2 = o['W'], o['g'], o['W2']
        MW = eta * (M @ W)
        return {(False, 2): (W @ g, W @ MW + alpha * W), (False, 1): (g, MW + alpha * np.eye(b.n_s, dtype=LD)),
                (False, 0): (o['q'], V @ MW + alpha * V), (True, 0): (W @ g, W @ MW + alpha * W + W2)}

    o, _ = R.eval_ref(b, z['G'], z['D'], NORMAL, alpha, 1.0, v=z['v'])
    md = modes(o, LD(1))
    for d_dv in (False, True):
        for proj in range(3):
            tag = 'n_ddv%d_p%d_' % (int(d_dv), proj)
            d, dd = md[(True, 0)] if d_dv else md[(False, proj)]
            check(tag + 'f', o['Q'])
            check(tag + 'd', d)
            check(tag + 'dd', dd)
    oe, _ = R.eval_ref(b, z['G'], z['D'], NORMAL, alpha, float(z['chi2_factor']), v=z['v'])
    d, dd = modes(oe, LD(float(z['chi2_factor'])))[(False, 2)]
    check('n_eta_f', oe['Q'])
    check('n_eta_d', d)
    check('n_eta_dd', dd)
    check('b_f', o['Q'])
    check('b_d', o['g'])
    check('b_dd', M @ o['W'])
    op, _ = R.eval_ref(b, z['G'], z['D'], PLUSMINUS, alpha, 1.0, v=z['v_pm'])
    mp = modes(op, LD(1))
    for d_dv in (False, True):
        tag = 'pm_ddv%d_p2_' % int(d_dv)
        d, dd = mp[(True, 0)] if d_dv else mp[(False, 2)]
        check(tag + 'f', op['Q'])
        check(tag + 'd', d)
        check(tag + 'dd', dd)
    # the component functions
    for pre, oo, kind in (('n_', o, NORMAL), ('pm_', op, PLUSMINUS)):
        check(pre + 'H', oo['H'])
        check(pre + 'dH_dv', oo['w'][:, None] * V)
        check(pre + 'chi2', oo['chi2'])
        check(pre + 'S', oo['S'])
        check(pre + 'dS_dH', -oo['u'])
        check(pre + 'ddS_diag', -1 / oo['w'])
        check(pre + 'dchi2_dH', 2 * (b.Ke.T @ (b.Ke @ oo['H'] - np.asarray(z['G'], dtype=LD) / b.err)))
        # H_of_v.inv: V^T safelog(...) of the image, the u of the input_is_H branch
        oh, _ = R.eval_ref(b, z['G'], z['D'], kind, alpha, 1.0, H=z[pre + 'H'])
        check(pre + 'v_of_H', V.T @ oh['u'])
        assert rel(oh['S'], z[pre + 'S']) < TOL and rel(oh['chi2'], z[pre + 'chi2']) < TOL
    assert set(worst) == set(k for k in z.files if k.startswith(('n_', 'pm_', 'b_'))), 'an entry of the fixture is not compared'
    print('worst relative deviation from derivs.npz: %.2e (%s)' % (max(worst.values()), max(worst, key=worst.get)))


def test_reference_reproduces_the_entropy_fixture():
    z = np.load(os.path.join(GOLD, 'plusminus_entropy.npz'))
    for kind, pre in ((PLUSMINUS, ''), (NORMAL, 'normal_')):
        o, _ = R.entropy_ref(kind, z['A'], z['D'])
        assert rel(o['S'][0], z[pre + 'f']) < 1e-11
        assert rel(o['d'][0], z[pre + 'd']) < 1e-11
        assert rel(o['dd'][0], z[pre + 'dd_diag']) < 1e-11


# ---------------------------------------------------------------------------------------------------------------------
#  2. a binary64 restatement of the kernel's arithmetic, with seeded faults
# ---------------------------------------------------------------------------------------------------------------------

FAULTS = ('last_row', 'odd_tail', 'no_cperp', 'Hm_sign', 'D_row', 'V_f32', 'tile', 'skip_Q', 'alpha_index', 'chol_col')


def fault_acts(fault, n_s, n_omega, audit):
    if fault in ('alpha_index', 'chol_col'):
        return audit and (fault == 'alpha_index' or n_s > 1)
    if audit:
        return False
    # (n_omega = 1: V = +-1 is a binary32 number; n_s = 1: Q = 1)
    return {'odd_tail': n_s % 2 == 1, 'tile': n_s > 16, 'skip_Q': n_s > 1, 'V_f32': n_omega > 1}.get(fault, True)


@functools.lru_cache(maxsize=None)
def whiten64(n_s, n_omega, ds):
    """build_dataset of maxent_hip.hip in binary64: (identity_q, Q, c, Uhat)"""
    c = R.make_case(n_s, n_omega)
    U, err = c.Us[ds], c.err[ds] * np.ones(c.Us[ds].shape[0])
    if not c.rotated[ds]:
        return True, None, c.S / err[0], U
    Uhat, cc, Q = R.jacobi_svd((U * c.S[None, :]) / err[:, None], dtype=np.float64)
    return False, Q, np.maximum(cc, 1e-150 * cc.max()), Uhat


class Model(object):
    """eval_kernel, mxe_eval_batch and mxe_audit in binary64 numpy (numpy's order of summation, not the kernel's)"""

    def __init__(self, case, faults=()):
        self.c, self.f = case, frozenset(faults)
        self.ds = []
        for d in range(3):
            ident, Q, cc, Uhat = whiten64(case.n_s, case.n_omega, d)
            Vp = case.V if ident else np.dot(case.V, Q)
            if 'V_f32' in self.f:
                Vp = Vp.astype(np.float32).astype(np.float64)
            self.ds.append((ident, Q, cc, Uhat, Vp))
        self.ghat, self.cperp = [], []
        for e, d in enumerate(ELEM_DS):
            Uhat = self.ds[d][3]
            Gt = case.G[e] / (case.err[d] * np.ones(Uhat.shape[0]))
            gh = np.dot(Uhat.T, Gt)
            r = Gt - np.dot(Uhat, gh)
            self.ghat.append(gh)
            self.cperp.append(0.0 if 'no_cperp' in self.f else float(np.dot(r, r)))

    def point(self, e, a, x, input_is_H, eta, whitened_x=False):
        """one workgroup: everything in the whitened basis"""
        f, ns, nw = self.f, self.c.n_s, self.c.n_omega
        ident, Q, cc, Uhat, Vp = self.ds[ELEM_DS[e]]
        kind = ELEM_KIND[e]
        D = self.c.D[e - 1 if ('D_row' in f and e > 0) else e]
        rot = not (ident or 'skip_Q' in f)
        rows = nw - 1 if 'last_row' in f else nw
        o = {}
        with np.errstate(all='ignore'):
            if input_is_H:
                H = np.array(x, dtype=float)
                vq = np.zeros(ns)
                if kind == NORMAL:
                    w, r = H, H / D
                else:
                    w = np.sqrt(H * H + (2 * D) ** 2)
                    r = (H + w) / (2 * D)
                u = np.log(np.where(np.abs(r) > 1e-100, r, 1e-100))
                Hp, Hm = (H, 0 * H) if kind == NORMAL else (0.5 * (w + H), 0.5 * (w - H))
            else:
                vq = np.dot(Q.T, x) if (rot and not whitened_x) else np.array(x, dtype=float)
                nu = ns - 1 if ('odd_tail' in f and ns % 2 == 1) else ns
                u = np.dot(Vp[:, :nu], vq[:nu])
                Hp = D * np.exp(u)
                Hm = D * np.exp(-u) if kind == PLUSMINUS else 0 * Hp
                H, w = Hp - Hm, Hp + Hm
            if kind == NORMAL:
                S = np.sum(Hp - D - Hp * u)
            else:
                S = np.sum((Hp - D - Hp * u) + ((Hm - D - Hm * u) if 'Hm_sign' in f else (Hm - D + Hm * u)))
            h = np.dot(Vp[:rows].T, H[:rows])
            rho = cc * h - self.ghat[e]
            chi2 = float(np.dot(rho, rho)) + self.cperp[e]
            t1, t2 = eta * cc * rho, a * vq
            g = t1 + t2
            den = np.abs(t1) + np.abs(t2)
            o['gmax'] = float(np.max(np.where(den > 0, np.abs(g) / np.where(den > 0, den, 1.0), 0.0)))
            q = np.dot(Vp, g)
            W = np.dot(Vp[:rows].T * w[None, :rows], Vp[:rows])
            W2 = np.dot(Vp[:rows].T * (q * H)[None, :rows], Vp[:rows])
            if 'tile' in f and ns > 16:
                W[16:32, 0:16] = 0.0                    # (the tile below the diagonal is what the mirror fills)
            o.update(Q=0.5 * eta * chi2 - a * S, chi2=chi2, S=S, H=H, u=u, w=w, q=q)
            o['_white'] = dict(W=W.copy(), rho=rho, vq=vq, cc=cc, Vp=Vp, w=w, H=H)
            if rot:
                h, g, W, W2 = np.dot(Q, h), np.dot(Q, g), np.dot(Q, np.dot(W, Q.T)), np.dot(Q, np.dot(W2, Q.T))
            o.update(h=h, g=g, W=W, W2=W2)
        return o

    def rotate(self, elem_of_chain, v, to_whitened):
        """[n_chain][n_alpha][n_s] between the caller's basis and the whitened one: v' = Q^T v (the upload), v = Q v' (the fetch)"""
        out = np.array(v, dtype=float)
        for ch, e in enumerate(elem_of_chain):
            ident, Q = self.ds[ELEM_DS[e]][:2]
            if not ident:
                out[ch] = np.dot(v[ch], Q) if to_whitened else np.dot(v[ch], Q.T)
        return out

    def audit(self, elem_of_chain, alpha, vq):
        """mxe_audit: [n_chain][n_alpha]; ``vq`` is the v' the chain kernel left on the device (``dout_v``)"""
        nc, na = alpha.shape
        corr, gmax = np.empty((nc, na)), np.empty((nc, na))
        for prob in range(nc * na):
            ch, ia = divmod(prob, na)
            e = elem_of_chain[ch]
            a = alpha.flat[prob // na] if 'alpha_index' in self.f else alpha.flat[prob]
            o = self.point(e, a, vq[ch, ia], False, 1.0, whitened_x=True)
            wh = o['_white']
            cc = wh['cc']
            B = cc[:, None] * wh['W'] * cc[None, :] + a * np.eye(len(cc))
            try:
                L = np.linalg.cholesky(B)
            except np.linalg.LinAlgError:
                corr[ch, ia], gmax[ch, ia] = np.nan, o['gmax']
                continue
            if 'chol_col' in self.f:
                L[1:, 0] = 0.0          # (the first: behind the strongest direction B is close to alpha I, its columns too)
            rhs = wh['rho'] + a * wh['vq'] / cc
            z = np.array(rhs)                   # two triangular solves, column oriented as in the kernel
            for j in range(len(z)):
                z[j] /= L[j, j]
                z[j + 1:] -= L[j + 1:, j] * z[j]
            for j in range(len(z) - 1, -1, -1):
                z[j] /= L[j, j]
                z[:j] -= L[j, :j] * z[j]
            du = np.dot(wh['Vp'], cc * z)
            corr[ch, ia] = np.linalg.norm(wh['w'] * du) / np.linalg.norm(wh['H'])
            gmax[ch, ia] = o['gmax']
        return corr, gmax


def gates_left(case, model, eta, input_is_H):
    """names of the outputs of any problem that leave their gate, and the worst error / (eps scale) per output"""
    ref = R.case_reference(case.n_s, case.n_omega, eta, input_is_H)
    left, worst = set(), dict((k, 0.0) for k in OUTPUTS)
    x = case.Himg if input_is_H else case.v
    for p in range(case.P):
        o = model.point(int(case.elem[p]), case.alpha[p], x[p], input_is_H, eta)
        ro, rs, C = ref[p]
        for k in OUTPUTS:
            ratio = R.worst_ratio(o[k], ro[k], rs[k])
            worst[k] = max(worst[k], ratio / C[k])
            if not ratio <= C[k]:
                left.add(k)
    return left, worst


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: '%dx%d' % s)
def test_restatement_passes_and_every_fault_is_caught(shape):
    case = R.make_case(*shape)
    runs = [(eta, is_H) for eta in R.ETAS for is_H in (False, True)]
    clean = Model(case)
    for eta, is_H in runs:
        left, worst = gates_left(case, clean, eta, is_H)
        print('%s eta=%.1f H=%d worst error / gate:' % (shape, eta, is_H),
              ' '.join('%s %.3f' % (k, worst[k]) for k in OUTPUTS))
        assert not left, (shape, eta, is_H, left, worst)
    for fault in FAULTS:
        if not fault_acts(fault, shape[0], shape[1], audit=False):
            continue
        model = Model(case, (fault,))
        caught = set()
        for eta, is_H in runs[:2]:
            caught |= gates_left(case, model, eta, is_H)[0]
        assert caught, (shape, fault, 'passes every gate')


# ---------------------------------------------------------------------------------------------------------------------
#  3. the audit: its cases, its gate, its faults
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def audit_points(n_s, n_omega, loose):
    """v of the oracle's alpha_chain under the options of the device test, in the caller's basis: [4][6][n_s]"""
    case = R.make_case(n_s, n_omega)
    opts = sform.KernelOptions(tol_h=1e-2, tol_d=0.0, tol_relq=0.0, stop_estimate=False) if loose else sform.KernelOptions()
    v = np.empty((len(ELEM_DS), len(R.AUDIT_ALPHAS), n_s))
    for e, ds in enumerate(ELEM_DS):
        basis = sform.Basis(case.Us[ds], case.S, case.V, case.err[ds])
        el = sform.Element(basis, case.G[e], case.D[e], 'normal' if ELEM_KIND[e] == NORMAL else 'plusminus')
        out = sform.alpha_chain(basis, el, R.AUDIT_ALPHAS, basis.from_v(R.audit_v0(case)), opts)
        v[e] = np.array([basis.to_v(x) for x in out['v']])
    return v


@pytest.mark.parametrize('shape', R.AUDIT_SHAPES, ids=lambda s: '%dx%d' % s)
def test_audit_cases_gate_and_faults(shape):
    case = R.make_case(*shape)
    elem = list(range(len(ELEM_DS)))
    alpha = np.tile(R.AUDIT_ALPHAS, (len(elem), 1))
    clean = Model(case)
    for loose in (True, False):
        # as on the device: the chains end at a v' in the whitened basis, which the audit reads; the caller fetches Q v'
        vq = clean.rotate(elem, audit_points(shape[0], shape[1], loose), to_whitened=True)
        v = clean.rotate(elem, vq, to_whitened=False)
        cref, gref, ggate = R.audit_reference(shape[0], shape[1], elem, alpha, v)
        print(shape, 'loose' if loose else 'default', 'corr_ref:', np.array2string(cref, precision=1))
        if loose:
            inside = np.sum((cref >= 1e-6) & (cref <= 1e-1))
            assert 3 * inside >= cref.size, ('the loose runs stop too close to (or too far from) the minimiser', cref)
        else:
            assert cref.max() < 1e-7, cref

        def left(model):
            corr, gmax = model.audit(elem, alpha, vq)
            bad_c = ~(np.abs(corr - cref) <= AUDIT_R * cref + AUDIT_F)
            bad_g = ~(np.abs(gmax - gref) <= ggate)
            return bad_c, bad_g, corr

        bad_c, bad_g, corr = left(clean)
        print('   worst |corr - ref| / ref: %.2e   worst |corr - ref|: %.2e' % (
            np.max(np.abs(corr - cref) / cref), np.max(np.abs(corr - cref))))
        assert not bad_c.any() and not bad_g.any(), (shape, loose, corr, cref)
        for fault in ('alpha_index', 'chol_col'):
            bad_c, bad_g, corr = left(Model(case, (fault,)))
            if loose:
                assert bad_c.any(), (shape, fault, 'passes the gate of corr')
