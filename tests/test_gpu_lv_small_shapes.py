"""chain_kernel_lv (mxe_kernel_lv.hip.h) at the shapes where its code changes, in both of its roles: the launch of a binary32
request (precision = F32) and the first pass of a binary64 launch (lds_basis = 1).  tests/test_gpu_lds_basis.py runs it at
n_omega = 200 and 500 with n_s = 51 ... 56 only; here:

    rows of V^T in LDS    NSL = max(32, n_s rounded up to 8), zero rows behind n_s: n_s = 5 ... 64
    tiles of h            nth = (n_s + 15) / 16 and vcol clamped to row NSL - 1: n_s = 32 / 33, 40 / 41, 48 / 49, 56 / 57
    halves and quarters   n_omega_pad = 128 (16 live lanes in the row pass, two K = 32 steps), 256, 384 (48 lanes, six steps), 512
    rows behind n_omega   129 in 256, 200 in 256, 300 in 384
    the alpha table       LV_ACAP = 16 entries: pieces of 16 (table), 17 and 40 alphas (mesh from memory), a piece led over 20
                          entries of the mesh, ladders of 8 + 1 and -- cut to the table -- 15 + 1 entries

The job is the 3 x 3 matrix of tests/test_gpu_lockstep_small_shapes.py -- normal entropy on the diagonal, plus-minus off it, one
data set: nine scans, the last workgroup holds one chain beside three empty slots -- on a basis cut to the wanted n_s: U, V the
leading singular vectors of a fermionic kernel, S prescribed, K = U S V^T, as tests/test_gpu_factor.py does, so that the oracle's
Problem, the truth and the device see one problem.  S falls by 10^-0.15 per direction down to S_31 = 2.2e-5 and by 2 % per direction
from S_32 = 1e-5 on: c_32 = S_32 / sigma = 1e-2, so the criterion that keeps a launch with n_s > 32 in this kernel,
c_32^2 max(1, sum D) / alpha_min <= 1e-3 (choose_precision), holds on every fine mesh (alpha_min = 0.8: 1.25e-4), and the
directions 32 ... 63 still count: at the minimiser alpha v_k = -c_k rho_k with ghat_k ~ N(0, 1), so each of them moves u = V v by
~ c_k / alpha = 5e-3 ... 1e-2 at the last alpha -- a row of V^T that the row pass drops or reads from the wrong place fails the
gates on H (a build whose row pass stops eight directions early fails 23 of the 34 cases); what the tiles of h beyond the active
block are for is checked on v itself (gate()).  The coarse mesh goes down to alpha = 8e-3 and runs with 32 directions, where the criterion does not apply.
tools/plan_dump.cpp gives lv_mode 1 / 2 for every case below; the kernel that ran is asserted by name.

Gates (the project's own: DESIGN 4d and 4h, tests/test_gpu_lds_basis.py): against the extended-precision fixed point reached from
the oracle's iterate (tests/anchor.py) at the first, middle and last alpha of a normal and a plus-minus element, and against the
one-chain binary64 kernel on the same context for every problem.  binary32: H within 1e-4 of both, device audit < 1e-4, chi2 to
2e-3.  Two-pass: 1e-6 against the truth, audit < 1e-6, H within 1e-7 of the binary64 kernel, chi2 to 1e-7.  Every alpha of a fine
mesh converges (the oracle does on each of them: asserted on the scans it runs); on the coarse mesh the flags are those of the
one-chain kernel and every alpha that converged is gated."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anchor                                                # noqa: E402
from maxent_amd import device, hostprep                      # noqa: E402
from oracle import ref_numpy as R                            # noqa: E402

pytestmark = pytest.mark.gpu

N_TAU, BETA, HALF_WIDTH, SIGMA = 80, 10.0, 5.0, 1e-3
LV_ACAP = 16
SHAPES = [(128, 5), (128, 16), (129, 31), (200, 32), (200, 33), (300, 40), (300, 41), (384, 48), (384, 49), (300, 57), (300, 64),
          (512, 56)]
ROLES = ('f32', 'two_pass')
ELEMS = [(i, j) for i in range(3) for j in range(3)]
TRUTH_ELEMS = (0, 1)                     # (0, 0): normal entropy; (0, 1): plus-minus


def log_mesh(n, hi, lo):
    """alpha~ from hi down to lo on n points, times the data points (what the reference iterates on)"""
    return N_TAU * hi * (lo / hi) ** (np.arange(n) / (n - 1.0))


def dense_tail_mesh():
    """36 alphas from 1e4 down to the last 6 % of the logarithmic range (a factor 1.42 apart), then 20 inside it: the single alphas
    of the guarded tail of a normal-entropy scan are led by the last alpha above it over up to 20 entries of the mesh"""
    top = 1e-2 * 1e6 ** 0.06
    return np.concatenate([log_mesh(36, 1e4, 1.02 * top), log_mesh(20, top / 1.02, 1e-2)])


# name -> (mesh, alpha_split, fine)
MESHES = {
    'fine': (log_mesh(40, 1e4, 1e-2), 0, True),                       # the library's own cut: pieces by cost, a led tail
    'table': (log_mesh(16, 1e3, 1.0), 1, True),                       # one piece of 16 alphas per scan: the table, full
    'memory': (log_mesh(17, 1e3, 1.0), 1, True),                      # 17: one more than the table holds
    'long': (log_mesh(40, 1e4, 1e-2), 1, True),                       # 40: nine pieces, the third workgroup holds one beside three empty slots
    'led': (dense_tail_mesh(), 28, True),                             # pieces of two alphas, a tail led over 2 ... 20 entries
    'ascending': (log_mesh(40, 1e4, 1e-2)[::-1].copy(), 5, True),     # pieces of 8: those below N_data / 4 walk down a ladder first
    'coarse': (log_mesh(4, 1e2, 1e-4), 0, False),                     # ladders of 8 rungs (alpha~ = 1e-2) and of 15 where 18 were wanted (1e-4)
}


SAME_MESH = dict(long='fine')             # (one reference and one truth for both)


def rel_l2(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


class Job(object):
    def __init__(self, n_omega, n_s):
        tau = np.linspace(0.0, BETA, N_TAU)
        w = np.linspace(-HALF_WIDTH, HALF_WIDTH, n_omega)
        Kf = np.exp(-np.outer(tau, w) - np.logaddexp(0.0, -BETA * w)[None, :])
        U, _, Vt = np.linalg.svd(Kf, full_matrices=False)
        k = np.arange(n_s)
        self.U, self.S, self.V = U[:, :n_s].copy(), np.where(k < 32, 10.0 ** (-0.15 * k), 1e-5 * 0.98 ** (k - 32)), Vt[:n_s].T.copy()
        self.K = np.dot(self.U * self.S, self.V.T)
        self.delta = w[1] - w[0]
        self.D = np.full(n_omega, 1.0 / n_omega)
        peaks = [0.6 * np.exp(-(w - 1.0 + 0.4 * i) ** 2 / 0.5) + 0.4 * np.exp(-(w + 1.5 - 0.3 * i) ** 2 / 0.8) + 1e-4 for i in range(3)]
        rng = np.random.RandomState(77)
        self.G = []
        for i, j in ELEMS:
            H = peaks[i] * self.delta if i == j else 0.3 * np.sqrt(peaks[i] * peaks[j]) * np.sin(1.3 * w + i - j) * self.delta
            self.G.append(np.dot(self.K, H))
        noise = SIGMA * rng.randn(3, 3, N_TAU)
        noise = 0.5 * (noise + noise.transpose(1, 0, 2))
        self.G = [g + noise[i, j] for g, (i, j) in zip(self.G, ELEMS)]
        self.kinds = [device.ENTROPY_NORMAL if i == j else device.ENTROPY_PLUSMINUS for i, j in ELEMS]
        self.v0 = np.stack([hostprep.initial_v(self.V, self.D, self.delta, k) for k in self.kinds])

    def context(self):
        ctx = device.DeviceContext(self.U, self.S, self.V)
        ds = ctx.add_dataset(SIGMA * np.ones(N_TAU))
        ctx.set_elements([ds] * 9, self.G, np.tile(self.D, (9, 1)), self.kinds)
        return ctx

    def problem(self, e):
        ent = 'normal' if self.kinds[e] == device.ENTROPY_NORMAL else 'plusminus'
        return R.Problem(self.K, self.U, self.S, self.V, self.G[e], SIGMA * np.ones(N_TAU), self.D, entropy=ent), ent


@functools.lru_cache(maxsize=None)
def job(n_omega, n_s):
    return Job(n_omega, n_s)


@functools.lru_cache(maxsize=None)
def truths(n_omega, n_s, mesh_name):
    """{element: {alpha index: H of the extended-precision fixed point}} at the first, middle and last alpha, reached from the
    oracle's own scan -- which has to converge at every alpha of a fine mesh"""
    j = job(n_omega, n_s)
    alphas, _, fine = MESHES[mesh_name]
    rows = (0, len(alphas) // 2, len(alphas) - 1)
    out = {}
    for e in TRUTH_ELEMS:
        p, ent = j.problem(e)
        out[e], ref = anchor.truth_rows(p, j.delta, alphas, N_TAU, rows, ent)
        assert ref['converged'].all() or not fine, ('the oracle does not converge on this problem', n_omega, n_s, mesh_name, e)
    return out


def solve(ctx, alphas, v0, **opts):
    ctx.upload_chains(np.arange(9), alphas, v0, device.default_opts(**opts))
    ctx.launch()
    kernel = ctx.last_launch_info()['kernel']
    first = ctx.fetch(want_v=False, want_H=False)       # the records of the launch alone
    left = ctx.finish()                  # (alphas the launch gave up on, solved again by the one-chain kernel)
    out = ctx.fetch(want_v=True, want_H=True)
    out['H'] = np.array(out['H'])
    out['kernel'], out['left'] = kernel, left
    out['launch_evals'], out['launch_converged'] = first['n_evals'].copy(), first['converged'].copy()
    out['audit'] = ctx.audit()['corr']
    out['depth'] = ctx.launch_depth()
    return out


@functools.lru_cache(maxsize=None)
def reference(n_omega, n_s, mesh_name):
    """the one-chain binary64 kernel, every scan in one piece"""
    j = job(n_omega, n_s)
    alphas, _, _ = MESHES[mesh_name]
    ctx = j.context()
    try:
        a = solve(ctx, alphas, j.v0, chains_per_wg=1, alpha_split=1, lds_basis=2)
    finally:
        ctx.close()
    assert a['kernel'].startswith('mxe::chain_kernel<') and 'double' in a['kernel'], a['kernel']
    return a


def role_opts(role):
    return dict(precision=device.PRECISION_F32) if role == 'f32' else dict(lds_basis=1)


def run(n_omega, n_s, mesh_name, role):
    j = job(n_omega, n_s)
    alphas, split, _ = MESHES[mesh_name]
    ctx = j.context()
    try:
        return solve(ctx, alphas, j.v0, alpha_split=split, **role_opts(role))
    finally:
        ctx.close()


def gate(n_omega, n_s, mesh_name, role, o):
    label = 'n_omega=%d n_s=%d %s %s' % (n_omega, n_s, mesh_name, role)
    alphas, _, fine = MESHES[mesh_name]
    if role == 'f32':
        assert o['kernel'] == 'mxe::chain_kernel_lv', (label, o['kernel'])
        tol_truth, tol_audit, tol_H, tol_chi2 = 1e-4, 1e-4, 1e-4, 2e-3
    else:
        assert o['kernel'].startswith('mxe::chain_kernel_lv + mxe::chain_kernel_mc<32'), (label, o['kernel'])
        tol_truth, tol_audit, tol_H, tol_chi2 = 1e-6, 1e-6, 1e-7, 1e-7
    a = reference(n_omega, n_s, SAME_MESH.get(mesh_name, mesh_name))
    ok = o['converged'].astype(bool)
    e_H = rel_l2(o['H'][ok], a['H'][ok])
    e_chi2 = np.abs(o['chi2'][ok] / a['chi2'][ok] - 1)
    e_truth = {}
    for e, rows in truths(n_omega, n_s, SAME_MESH.get(mesh_name, mesh_name)).items():
        for ia, Ht in rows.items():
            if ok[e, ia]:
                e_truth[(e, ia)] = anchor.rel_l2_checked(o['H'][e, ia], Ht)
    print('%s: %s; converged %d of %d (one-chain kernel: %d), %d left to the finishing pass; H against truth %.2e, against the one-chain kernel %.2e; chi2 %.2e; '
          'audit %.2e; evaluations max %d; rounds %s' % (label, o['kernel'], ok.sum(), ok.size, a['converged'].sum(), o['left'], max(e_truth.values()),
                                                         e_H.max(), e_chi2.max(), np.nanmax(o['audit'][ok]), o['n_evals'].max(),
                                                         o['depth']['max_rounds']))
    assert np.array_equal(o['converged'], a['converged']), (label, np.argwhere(o['converged'] != a['converged']))
    if fine:
        assert ok.all() and o['left'] == 0, (label, o['left'], np.argwhere(~ok))         # (nothing handed to another kernel)
    assert ok.any() and len(e_truth) > 0
    for key in ('H', 'chi2', 'Q', 'S'):
        assert np.isfinite(o[key][ok]).all(), (label, key)
    assert max(e_truth.values()) < tol_truth, (label, e_truth)
    assert np.all(np.isfinite(o['audit'][ok])) and o['audit'][ok].max() < tol_audit, (label, o['audit'][ok].max())
    assert e_H.max() < tol_H, (label, e_H.max())
    np.testing.assert_allclose(o['chi2'][ok], a['chi2'][ok], rtol=tol_chi2)
    if n_s > 32 and role == 'f32':
        # The directions beyond the active block, where this kernel's v is the caller's result.  Their Newton step is the diagonal
        # one, v_k = -c_k (c_k h_k - ghat_k) / alpha, so what the third and fourth tile of h = V^T H contribute to H is bounded by
        # the criterion itself (c_k^2 / alpha <= 1e-3) and lies below the classes above: builds with nth one short (n_s = 33, 49)
        # or vcol clamped one row low (n_s = NSL) pass every gate on H.  But ALL of v_k depends on h_k.  The returned v_k is that
        # formula at the H of the iterate before, which the stopping rule leaves within LV_FLOOR = 2e-5 of the last; an H within
        # tol_H of the reference's gives |dh_k| <= tol_H |H| (the columns of V have unit length); hence
        # |dv_k| <= c_k^2 (tol_H + LV_FLOOR) |H| / alpha.  A tile of h that is not summed, or summed from the wrong row of V^T,
        # misses that by |h_k| / (1.2e-4 |H|): those two builds fail here at exactly their shapes.
        c = job(n_omega, n_s).S[32:] / SIGMA
        bound = c ** 2 * (tol_H + 2e-5) * np.linalg.norm(a['H'], axis=-1)[..., None] / alphas[None, :, None]
        dv = np.abs(o['v'][..., 32:] - a['v'][..., 32:])
        print('   v_k, k >= 32, against the one-chain kernel: worst |dv_k| / bound %.3f' % (dv / bound)[ok].max())
        assert (dv[ok] <= bound[ok]).all(), (label, (dv / bound)[ok].max())


@pytest.mark.parametrize('role', ROLES)
@pytest.mark.parametrize('n_omega,n_s', SHAPES)
def test_every_shape_of_chain_kernel_lv(n_omega, n_s, role):
    """the 3 x 3 job on 40 alphas: every scan one piece (nine pieces in three workgroups, the last with one chain beside three
    empty slots; alphas read from memory), and cut by the library's own rule (168 pieces by cost, alphas from the table, a led tail)"""
    for mesh_name in ('long', 'fine'):
        gate(n_omega, n_s, mesh_name, role, run(n_omega, n_s, mesh_name, role))


# the pieces, at the shape with a zeroed tail of rows (300 in 384), three tiles of h and a clamped vcol (n_s = 41, NSL = 48)
PIECES_SHAPE = (300, 41)


@pytest.mark.parametrize('role', ROLES)
@pytest.mark.parametrize('mesh_name', ['table', 'memory', 'led', 'ascending'])
def test_pieces_within_and_beyond_the_alpha_table(mesh_name, role):
    """pieces of 16 alphas (the slot's table, full) and of 17 (alpha_at reads the mesh from memory; 40: the test above), single
    alphas led over up to 20 entries of the mesh (the walk reads it from memory at negative indices), pieces of an ascending scan"""
    gate(*PIECES_SHAPE, mesh_name, role, run(*PIECES_SHAPE, mesh_name, role))


# Evaluations a laddered alpha may take in chain_kernel_lv beyond what it takes in chain_kernel_mc on the same rungs, and converged
# laddered alphas it may fall short by.  First measurement with the ladders cut to the table (the launch alone, nine scans; alpha = 0.8
# after 7 rungs | alpha = 8e-3 after 15, '-': given up during the walk or at the alpha, left to the finishing pass):
#     chain_kernel_mc        4 4 4 4 4 4 4 4 4 | 42  -  -  - 4  - 12  -  -
#     chain_kernel_lv, F32   4 4 4 4 4 4 4 4 4 | 44  -  -  - 6  -  -  -  -         at most 2 more; headroom for its stopping rule
#     ... first pass         5 5 5 5 5 5 5 5 5 | 44 25  9 39 7 46 17 36  -         (LV_FLOOR, the 3e-5 |Q| margin of its descent test): 2
#                                                                                  two-pass: at most 5 more (of which the second pass
#                                                                                  adds one step and the evaluation that confirms it)
# (with its own 18 rungs of 1.56 to alpha = 8e-3 chain_kernel_mc took 4 - 9 - 4 - 13 - 4: what the table of 16 costs is the ladder's
#  length, not the kernel -- DESIGN 4h)
LADDER_MARGIN = dict(f32=2 + 2, two_pass=5 + 2)
LADDER_SHORT = dict(f32=1 + 1, two_pass=0)


@pytest.mark.parametrize('role', ROLES)
def test_laddered_pieces_are_walked(role, monkeypatch):
    """Four alphas from alpha~ = 1e2 down to 1e-4: the third and the fourth of every scan are pieces of their own that walk down a
    ladder from N_data / 4 = 20 -- 8 rungs to alpha = 0.8, and 15 to 0.008 where a ratio of 1.56 wants 18: 16 entries are what the
    slot's table holds, and rungs are walked from the table only (tests/test_launch_plan_host.py).  The launch as the library
    plans it passes the gates of the coarse mesh.  Then the walk itself: a ladder that is walked leaves its alpha a warm start, so
    the evaluations that alpha takes in the launch are compared with those of chain_kernel_mc (lds_basis = 2) on the same job AND
    the same rungs -- MXE_LADDER_RATIO = 1.685 makes both planners lay 7 and 15 of them.  An alpha that walks anything else starts
    cold five decades below the data: hundreds of evaluations in the one-chain kernel, none that converge within the 96 of a
    lock-step slot."""
    n_omega, n_s = 200, 32               # (alpha_min = 8e-3: with more than 32 directions the launch would leave this kernel)
    gate(n_omega, n_s, 'coarse', role, run(n_omega, n_s, 'coarse', role))
    monkeypatch.setenv('MXE_LADDER_RATIO', '1.685')
    o = run(n_omega, n_s, 'coarse', role)
    j = job(n_omega, n_s)
    alphas, split, _ = MESHES['coarse']
    ctx = j.context()
    try:
        m = solve(ctx, alphas, j.v0, alpha_split=split, lds_basis=2)
    finally:
        ctx.close()
    monkeypatch.delenv('MXE_LADDER_RATIO')
    assert m['kernel'].startswith('mxe::chain_kernel_mc<32') and 'lead' in m['kernel'], m['kernel']
    laddered = [i for i in range(1, len(alphas)) if alphas[i] < 0.25 * N_TAU and alphas[i - 1] / alphas[i] > 2.0]
    assert laddered == [2, 3]
    ev_lv, ev_mc = o['launch_evals'][:, laddered].T, m['launch_evals'][:, laddered].T
    ok_lv, ok_mc = o['launch_converged'][:, laddered].T.astype(bool), m['launch_converged'][:, laddered].T.astype(bool)
    print('evaluations of the laddered alphas in the launch (alpha x scan; converged), chain_kernel_lv as %s:\n%s\n%s\nchain_kernel_mc:\n%s\n%s'
          % (role, ev_lv, ok_lv.astype(int), ev_mc, ok_mc.astype(int)))
    gate(n_omega, n_s, 'coarse', role, o)
    both = ok_lv & ok_mc
    assert both[0].all() and both[1].any()                      # the short ladder always lands; the long one in some scans
    assert (ev_lv[both] <= ev_mc[both] + LADDER_MARGIN[role]).all(), (ev_lv, ev_mc)
    assert ok_lv.sum() >= ok_mc.sum() - LADDER_SHORT[role], (ok_lv.sum(), ok_mc.sum())
