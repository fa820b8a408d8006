"""The job and the cases of tests/test_newton_step_ref_host.py and tests/test_gpu_one_chain_builds.py: every reachable build of
the one-chain kernel (chain_kernel<NW, NAB, TS, GST>) at the shapes where its code changes.

The job is the Job of tests/test_gpu_lv_small_shapes.py -- U, V the leading n_s singular vectors of the fermionic kernel on
linspace(-5, 5, n_omega), K = U S V^T, D = 1 / n_omega, beta = 10, sigma = 1e-3, n_tau = max(80, n_s + 8), RandomState(77) --
with ONE normal-entropy and ONE plus-minus element (its elements (0, 0) and (0, 1)) and another spectrum:
S = logspace(0, -2, n_s), so that c = S / sigma runs from 1e3 down to 10 and EVERY direction enters the Newton matrix
c W c + alpha I at the alphas of the mesh (12 alphas, alpha_i = n_tau 10^(3 - 3 i / 11)): the step with the last direction
decoupled differs from the true one by 7.7e-5 ... 5.8e-2 of its length at n_omega <= 300 and by >= 1.2e-6 on the long meshes
(tests/test_newton_step_ref_host.py asserts 1e-6), where the spectra of the other GPU tests leave 1e-9 ... 1e-16.

Nothing here touches the device: the start vectors of the one-step test are the iterates of the numpy model of the kernel
(oracle/sform.alpha_chain, binary64, the full n_s block)."""
import functools

import numpy as np

from oracle import ref_numpy as R, sform as SF

BETA, HALF_WIDTH, SIGMA = 10.0, 5.0, 1e-3
N_ALPHA = 12
STEP_ROWS = (6, 11)                    # alpha indices of the one-step test
TRUTH_ROWS = (0, 6, 11)                # ... at which the scans are compared with the extended-precision fixed point
ENTROPIES = ('normal', 'plusminus')    # element 0, element 1  (device.ENTROPY_NORMAL = 0, ENTROPY_PLUSMINUS = 1)
STEP_MAX = 0.2                         # mxe_opts.step_max (default)


def n_tau_of(n_s):
    return max(80, n_s + 8)


def alpha_mesh(n_s):
    return n_tau_of(n_s) * 10.0 ** (3.0 - 3.0 * np.arange(N_ALPHA) / (N_ALPHA - 1.0))


class Job(object):
    def __init__(self, n_omega, n_s):
        self.n_omega, self.n_s, self.n_tau = n_omega, n_s, n_tau_of(n_s)
        tau = np.linspace(0.0, BETA, self.n_tau)
        w = np.linspace(-HALF_WIDTH, HALF_WIDTH, n_omega)
        Kf = np.exp(-np.outer(tau, w) - np.logaddexp(0.0, -BETA * w)[None, :])
        U, _, Vt = np.linalg.svd(Kf, full_matrices=False)
        self.U, self.S, self.V = U[:, :n_s].copy(), np.logspace(0.0, -2.0, n_s), Vt[:n_s].T.copy()
        self.K = np.dot(self.U * self.S, self.V.T)
        self.delta = w[1] - w[0]
        self.D = np.full(n_omega, 1.0 / n_omega)
        self.err = SIGMA * np.ones(self.n_tau)
        self.alphas = alpha_mesh(n_s)
        peaks = [0.6 * np.exp(-(w - 1.0 + 0.4 * i) ** 2 / 0.5) + 0.4 * np.exp(-(w + 1.5 - 0.3 * i) ** 2 / 0.8) + 1e-4 for i in range(2)]
        signals = [peaks[0] * self.delta, 0.3 * np.sqrt(peaks[0] * peaks[1]) * np.sin(1.3 * w + 0 - 1) * self.delta]
        noise = SIGMA * np.random.RandomState(77).randn(2, self.n_tau)
        self.G = [np.dot(self.K, H) + noise[e] for e, H in enumerate(signals)]
        self.c = self.S / SIGMA
        self.ghat = [np.dot(self.U.T, G / SIGMA) for G in self.G]
        self.basis = SF.Basis(self.U, self.S, self.V, self.err)
        assert self.basis.Q is None                      # (one error bar: the whitened basis IS (U, S / sigma, V))
        self.elements = [SF.Element(self.basis, G, self.D, ent) for G, ent in zip(self.G, ENTROPIES)]

    def problem(self, e):
        """the oracle's problem (its constructor builds n_omega x n_omega arrays: for the meshes the oracle runs on)"""
        return R.Problem(self.K, self.U, self.S, self.V, self.G[e], self.err, self.D, entropy=ENTROPIES[e])

    def initial_v(self, e):
        """the reference's start: v with H(v) = D delta (R.initial_v; plus-minus: H+ - H- = D delta)"""
        A = self.D * self.delta
        x = A / self.D if ENTROPIES[e] == 'normal' else (A + np.sqrt(A ** 2 + 4 * self.D ** 2)) / (2 * self.D)
        return np.dot(self.V.T, np.log(x))

    def values_at(self, e, v):
        """(H, chi2, S) at v as the reference evaluates them, with the full kernel (R.H_of_v, R.chi2_f, R.S_f)"""
        u = np.dot(self.V, v)
        if ENTROPIES[e] == 'normal':
            H = self.D * np.exp(u)
            S = np.sum(H - self.D - H * u)
        else:
            Hp, Hm = self.D * np.exp(u), self.D * np.exp(-u)
            H = Hp - Hm
            S = np.sum(Hp - self.D - Hp * u) + np.sum(Hm - self.D + Hm * u)
        return H, float(np.sum(((np.dot(self.K, H) - self.G[e]) / self.err) ** 2)), float(S)

    def sum_D(self, e):
        return self.D.sum() * (1.0 if ENTROPIES[e] == 'normal' else 2.0)


@functools.lru_cache(maxsize=None)
def job(n_omega, n_s):
    return Job(n_omega, n_s)


@functools.lru_cache(maxsize=None)
def model(n_omega, n_s, e):
    """the numpy model of the kernel over the mesh, warm, the full block: (its records, [(n_iter, n_evals, n_chol)] per alpha)"""
    j = job(n_omega, n_s)
    stats = []
    m = SF.alpha_chain(j.basis, j.elements[e], j.alphas, j.initial_v(e), SF.KernelOptions(), stats)
    return m, stats


# ---- the cases: (build as mxe_last_kernel_name spells it, options that ask for it, n_omega, n_s) ----
def _f64(nw):
    return 'mxe::chain_kernel<%d, 2, double>' % nw, dict(chains_per_wg=1, waves_per_chain=nw)


NAB2_SHAPES = [(128, 5),                         # n_act < 16
               (128, 16), (128, 17),             # class and Gram-tile edge 16 | 17
               (200, 24), (200, 25),             # class 24 | 32
               (129, 32), (200, 33),             # register solve | gj_solve_4w (NW = 4), fused chol_solve (NW = 1, 2); 129 pads to 256
               (300, 48), (300, 49),             # block edge of gj_solve_4w, three | four Gram tiles
               (300, 63),                        # last fused row
               (128, 64), (300, 64)]             # n_act == NP: unfused chol_solve
F32_SHAPES = [(128, 16), (200, 33), (300, 63), (128, 64)]
ONE_WAVE = dict(chains_per_wg=1, waves_per_chain=1)
CASES = []
for _nw in (1, 2, 4):
    CASES += [_f64(_nw) + s for s in NAB2_SHAPES]
# NAB = 4 in LDS (only n_omega <= 128 fits): fused, 6 pairs | 6 and 10 pairs of the VALU sweep | unfused
CASES += [('mxe::chain_kernel<1, 4, double>', ONE_WAVE) + s for s in [(128, 65), (128, 96), (128, 97), (128, 128)]]
# ... in device memory: (129, 65) has 33 staged Gram tiles of 4 rows, the last three rows zero
CASES += [('mxe::chain_kernel<1, 4, double, device-memory state>', ONE_WAVE) + s for s in [(129, 65), (300, 96), (300, 97), (300, 128)]]
CASES += [('mxe::chain_kernel<4, 2, double, device-memory state>', dict(chains_per_wg=1, waves_per_chain=4)) + s
          for s in [(3000, 33), (3000, 64)]]
for _nw in (1, 2, 4):
    # (precision: device.PRECISION_F32 = 1; lds_basis = 2 keeps the request out of chain_kernel_lv)
    CASES += [('mxe::chain_kernel<%d, 2, float>' % _nw, dict(chains_per_wg=1, waves_per_chain=_nw, precision=1, lds_basis=2)) + s
              for s in F32_SHAPES]
CASES += [('mxe::chain_kernel<4, 2, float, device-memory state>', dict(chains_per_wg=1, waves_per_chain=4, precision=1, lds_basis=2),
           6300, 64)]
SCAN_CASES = [c for c in CASES if c[2] < 3000]       # (the scans of the long meshes: test_frequency_mesh_beyond_the_lds)
SHAPES = sorted(set(c[2:] for c in CASES))
F32_STEP_SHAPES = sorted(set(c[2:] for c in CASES if 'float' in c[0]))
BUILDS = sorted(set(c[0] for c in CASES))


def case_id(case):
    name, _, n_omega, n_s = case
    return '%s-%dx%d' % (name[len('mxe::chain_kernel'):].replace(', ', '_').replace(' ', '_'), n_omega, n_s)


def find_case(name, n_omega, n_s):
    return [c for c in CASES if c[0] == name and c[2:] == (n_omega, n_s)][0]


# ---- the one-step references (tests/newton_step_ref.py), shared by the host test and the GPU test ----
@functools.lru_cache(maxsize=None)
def step_ref(n_omega, n_s, e, ia):
    """the undamped step at alpha index ``ia`` from the model's v of the alpha before, in extended precision:
    dict(v0, alpha, delta (longdouble), q = delta^T W delta)"""
    import newton_step_ref as N
    j = job(n_omega, n_s)
    v0 = model(n_omega, n_s, e)[0]['v'][ia - 1].copy()
    delta, q = N.newton_step(j.V, j.c, j.ghat[e], j.D, ENTROPIES[e], j.alphas[ia], v0, N.LD)
    return dict(v0=v0, alpha=j.alphas[ia], delta=delta, q=q)


@functools.lru_cache(maxsize=None)
def step_err(n_omega, n_s, e, ia, dtype, drop=None):
    """|step in ``dtype`` (with direction ``drop`` decoupled) - the extended-precision step| / |that step|"""
    import newton_step_ref as N
    j = job(n_omega, n_s)
    r = step_ref(n_omega, n_s, e, ia)
    d, _ = N.newton_step(j.V, j.c, j.ghat[e], j.D, ENTROPIES[e], r['alpha'], r['v0'], dtype, drop)
    return N.rel_err(d, r['delta'])


F64_STEP_GATE = 1e-9


def f32_step_gate(n_omega, n_s, e, ia):
    """the gate of a binary32 build on its step: ten times what the binary32 stream arithmetic itself costs this step"""
    return 10.0 * step_err(n_omega, n_s, e, ia, 'f32 stream')
