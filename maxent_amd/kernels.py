"""Kernels of the analytic continuation and their SVD staging (host side).

``G_i = sum_j K_ij H_j`` with ``H = A * delta_omega``.  The kernel matrix is
filled and decomposed once on the host with numpy/LAPACK; the truncated
factors ``U, S, V`` are what :class:`maxent_amd.device.DeviceContext` stages
in HBM.  Public names and semantics follow the reference's ``kernels`` module
(reference python/kernels.py:37-413): ``KernelSVD``, ``Kernel``,
``DataKernel``, ``TauKernel``, ``IOmegaKernel``, ``PreblurKernel``.  ``BosonicTauKernel`` and
``BosonicIOmegaKernel`` (susceptibilities: chi(tau), chi(i nu_n)) and ``LegendreKernel`` (Legendre coefficients G_l)
have no counterpart there.
"""

import numpy as np

from .preblur import get_preblur


class _one_blas_thread(object):
    """``threadpoolctl.threadpool_limits(1)`` where the package is there, nothing otherwise"""

    def __enter__(self):
        self._ctx = None
        try:
            from threadpoolctl import threadpool_limits
            self._ctx = threadpool_limits(limits=1)
            self._ctx.__enter__()
        except Exception:
            self._ctx = None
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


def _fingerprint(a):
    """64-bit content hash of a contiguous float array (xxhash where the package is there, zlib.crc32 + adler32 otherwise)"""
    a = np.ascontiguousarray(a)
    try:
        import xxhash
        return xxhash.xxh3_64_intdigest(memoryview(a).cast('B'))
    except Exception:
        import zlib
        m = memoryview(a).cast('B')
        return (zlib.crc32(m) << 32) | zlib.adler32(m)


class _Recent(object):
    """the few most recently used results of an expensive function of array CONTENTS (kernel fill, SVD): a new TauMaxEnt /
    ElementwiseMaxEnt on the grids of an earlier one -- every iteration of a self-consistency loop, both workers of an
    element-wise run -- fills and decomposes the same 200 x 500 matrix again (reference elementwise_maxent.py:170-221: one fresh
    SVD per ELEMENT; here it was one per object, 6.5-7.7 ms of the 13-15 ms a fresh object took).  Entries are found by a content
    hash and confirmed by comparing the arrays; what they hand out is shared and READ-ONLY.

    Contract (differs from the reference, where ``K.K``, ``K.K_delta``, ``K.U``, ``K.S``, ``K.V`` are private writable arrays):
    in-place edits such as ``K.K[...] *= x`` raise numpy's "assignment destination is read-only".  Code that wants to change
    a kernel assigns a NEW array (``kernel._K = kernel.K * x``) or works on ``np.array(kernel.K)``; README.md, "Differences a
    user of the reference will notice"."""

    def __init__(self, size=4):
        import collections
        import threading
        self._d, self._size, self._lock = collections.OrderedDict(), size, threading.Lock()

    def get(self, key, confirm):
        with self._lock:
            hit = self._d.get(key)
            if hit is not None and confirm(hit[0]):
                self._d.move_to_end(key)
                return hit[1]
        return None

    def put(self, key, witness, value):
        with self._lock:
            self._d[key] = (witness, value)
            while len(self._d) > self._size:
                self._d.popitem(last=False)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


_recent_svd = _Recent()
_recent_fill = _Recent()


class KernelSVD(object):
    """Matrix with a lazily computed thin SVD ``K = U diag(S) V^T``.

    ``V`` is stored as ``n_omega x n_s`` (reference kernels.py:53-64).
    """

    #: 'host' (numpy / LAPACK, the reference's path) or 'device'
    #: (``mxe_kernel_svd`` and its siblings: fill, preblur product and a preconditioned
    #: one-sided Jacobi SVD on the GPU; every kernel of this module implements ``_device_svd`` --
    #: the ones that know how they are filled are filled there, a DataKernel's matrix is sent)
    svd_backend = 'host'

    def __init__(self, K=None):
        self._U = self._S = self._V = None
        self._K = K
        self._last_threshold = None

    def _invalidate_svd(self):
        self._U = self._S = self._V = None

    def _device_svd(self):
        raise NotImplementedError('svd_backend="device" needs a Kernel of this module '
                                  '(a bare KernelSVD has no omega mesh)')

    def svd(self):
        if self._U is None:
            if self.svd_backend == 'device':
                self._U, self._S, self._V = self._device_svd()
            elif self.svd_backend == 'host':
                # (one BLAS thread: the decomposition of a few hundred rows is no faster on many -- 8 threads were
                #  slower than 1 in BASELINE.md -- and a BLAS pool that spins up on every core of the host burns the
                #  CPU quota of a container: the process then stalls for most of a scheduler period, 70 ms, at some
                #  later point of the run)
                K = np.ascontiguousarray(self.K, dtype=float)
                key = (K.shape, _fingerprint(K))
                hit = _recent_svd.get(key, lambda K0: K0.shape == K.shape and np.array_equal(K0, K))
                if hit is None:
                    with _one_blas_thread():
                        U, S, Vh = np.linalg.svd(K, full_matrices=False)
                    hit = (_frozen(U), _frozen(S), _frozen(Vh.transpose()))
                    _recent_svd.put(key, K.copy(), hit)
                self._U, self._S, self._V = hit
            else:
                raise ValueError("svd_backend must be 'host' or 'device'")
        return (self._U, self._S, self._V)

    @property
    def U(self):
        return self.svd()[0]

    @property
    def S(self):
        return self.svd()[1]

    @property
    def V(self):
        return self.svd()[2]

    @property
    def K(self):
        return self._K

    def reduce_singular_space(self, threshold=1.e-14):
        """Drop singular values below the ABSOLUTE ``threshold``
        (reference kernels.py:101-122); a later call with a smaller
        threshold recomputes the SVD."""
        if self._last_threshold is not None:
            if threshold is None or threshold < self._last_threshold:
                self._invalidate_svd()
        self._last_threshold = threshold
        keep = np.where(self.S >= threshold)[0]
        if len(keep) < len(self._S):             # nothing to drop: U, S, V stay the objects they are
            self._U = self._U[:, keep]
            self._S = self._S[keep]
            self._V = self._V[:, keep]
        return self


class Kernel(KernelSVD):
    """Kernel on an omega mesh with an optional left rotation ``T``
    (covariance eigenbasis; reference kernels.py:125-180)."""

    #: the matrix has been taken out of a rotation with fewer rows than columns by ``transform``: it is a projection
    #: of what its rotation says (``refill_unrotated`` mends it)
    _projected = False

    # ---- what a kind of kernel says about itself (read by _fill_values, _device_svd, PreblurKernel, TauMaxEnt._use_kernel)
    #: tag of a kind that fills its matrix itself, in the key of the fill cache: equal tau and i omega grids stay apart.
    kind = None
    #: whether beta enters the matrix: a new beta refills it (the Matsubara kernels only remember theirs)
    beta_in_matrix = True
    #: constructor arguments whose change makes another kernel, not a refill
    kind_params = ()
    #: whether the rows are ``[Re K ; Im K]`` and the data complex (:class:`_StackedRows`)
    stacked = False
    #: whether ``_device_entry`` is there: the device fills (or takes) and decomposes the matrix
    has_device_entry = False
    #: whether ``PreblurKernel.scan`` takes the kind
    scannable = False

    def __init__(self):
        super(Kernel, self).__init__()
        self.omega = None
        self._T = None

    @property
    def setter_kind(self):
        """the ``kind`` whose setters of TauMaxEnt keep this kernel: its own, or -- a kernel that does not fill itself,
        a DataKernel or a user's class -- that of G(tau) data"""
        return 'tau' if self.kind is None else self.kind

    @classmethod
    def _checked_args(cls, grid, **params):
        """the grid as a setter of TauMaxEnt assigns it (``TauMaxEnt._use_kernel``); a kind that validates its arguments
        raises here, before anything is changed"""
        return grid

    @property
    def rotation(self):
        """the absolute left rotation the matrix and U currently carry (None: unrotated)"""
        return self._T

    @property
    def K_delta(self):
        """K * delta_omega, never rotated: ``G_rec = K_delta A``."""
        return self._K_delta

    @property
    def data_variable(self):
        raise NotImplementedError('Use a subclass of Kernel')

    def parameter_change(self):
        self._fill_values()

    def _inputs(self, w):
        """what the matrix depends on besides the omega mesh ``w``, validated: a tuple of arrays and scalars.  It is the
        kind's part of the key of the fill cache and the arguments of :meth:`_compute`."""
        raise NotImplementedError('Use a subclass of Kernel')

    def _compute(self, w, *inputs):
        """the unrotated matrix on the mesh ``w`` from :meth:`_inputs`"""
        raise NotImplementedError('Use a subclass of Kernel')

    def _fill_values(self):
        """the unrotated matrix from the cache of recent fills or from ``_compute`` -- shared and read-only either way --,
        then the rotation the kernel carries again"""
        self._invalidate_svd()
        w = np.asarray(self.omega, dtype=float)
        inputs = self._inputs(w)
        delta = np.asarray(self.omega.delta, dtype=float)
        key = (self.kind, w.tobytes(), delta.tobytes()) + \
            tuple([x.tobytes() if type(x) is np.ndarray else x for x in inputs])
        hit = _recent_fill.get(key, lambda _: True)               # (the key IS the contents)
        if hit is None:
            K = self._compute(w, *inputs)
            hit = (_frozen(K), _frozen(K * delta[np.newaxis, :]))
            _recent_fill.put(key, None, hit)
        self._K, self._K_delta = hit
        self._K_unrotated = hit[0]
        T = self._T
        self._T = None
        self.transform(T)

    def _device_entry(self, preblur_b=0.0):
        """``(name, grid, scalars, n_rows)``: the C entry that fills and decomposes this kind, its row grid, the scalar
        arguments between ``delta`` and ``n_b`` in the entry's order, and the number of rows of the matrix"""
        raise NotImplementedError('svd_backend="device" needs a kernel of this module')

    def _device_svd(self, preblur_b=0.0):
        """U, S, V of the UNROTATED kernel from the device: everything the QR stage kept
        (singular values down to eps * sigma_max; the reference's LAPACK values below
        that are rounding noise), ``reduce_singular_space`` cuts as usual."""
        from . import device
        name, grid, scalars, n_rows = self._device_entry(preblur_b)
        r = device._kernel_svd(name, grid, scalars, np.asarray(self.omega, dtype=float), self.omega.delta,
                               [preblur_b], threshold=0.0, n_rows=n_rows)[0]
        return r['U'], r['S'], r['V']

    def refill_unrotated(self):
        """the unrotated matrix again, filled afresh: the way out of a rotation with fewer rows than columns, which
        ``transform(None)`` cannot undo (T^H T is a projection then)"""
        self._T = None
        self._projected = False
        self._fill_values()

    def fold(self, x):
        """a data-space vector or array (last axis = the rows of K) in the form of the data the kernel was made for;
        identity here, complex for :class:`IOmegaKernel`, whose rows are the stacked real and imaginary parts"""
        return x

    def unfold(self, x):
        """the inverse of :meth:`fold`"""
        return x

    def transform(self, T_):
        """Left-multiply K (and U) by ``T_``, given as the absolute rotation
        with respect to the unrotated kernel; ``None`` undoes it."""
        T = self._relative_rotation(T_, self._T)
        if T is None:
            return
        if self._T is not None and self._T.shape[0] != self._T.shape[1]:
            self._projected = True       # (T_old^H T_old is a projection: what follows is T_ times a projected K)
        self._T = T_
        self._U = np.dot(T, self.U)
        self._K = np.dot(T, self._K)

    @staticmethod
    def _relative_rotation(T_to, T_from):
        """the matrix that takes the kernel from rotation ``T_from`` to ``T_to``; None if there is
        nothing to do (the same rotation object, or unrotated to unrotated)"""
        if T_to is T_from:
            return None
        if T_to is None:
            return T_from.conjugate().transpose()
        if T_from is None:
            return T_to
        return np.dot(T_to, T_from.conjugate().transpose())


class DataKernel(Kernel):
    """Kernel given as a matrix (reference kernels.py:183-207)."""

    has_device_entry = True

    def __init__(self, data_variable, omega, K, svd_backend='host'):
        super(DataKernel, self).__init__()
        self._data_variable = data_variable
        self.omega = omega
        self._K = K
        self._K_delta = K * omega.delta[np.newaxis, :]
        self.svd_backend = svd_backend

    @property
    def data_variable(self):
        return self._data_variable

    def transform(self, T_):
        if self._T is None and not self._projected:
            self._K_unrotated = self._K          # (the matrix as it was given: transform assigns a new one)
        super(DataKernel, self).transform(T_)

    def refill_unrotated(self):
        if self._T is not None or self._projected:
            self._T = None
            self._projected = False
            self._invalidate_svd()
            self._K = self._K_unrotated

    def _device_entry(self, preblur_b=0.0):
        """the matrix as it stands (``mxe_kernel_svd_data``); with ``preblur_b`` > 0 the UNROTATED one -- the blur acts
        from the right, so the rotation is taken off the rows first"""
        K = np.asarray(self._K, dtype=float)
        if preblur_b > 0.0 and self._T is not None:
            K = np.dot(self._T.conjugate().transpose(), K)
        return 'mxe_kernel_svd_data', K, (), len(K)


def _tau_and_beta(kernel):
    """the tau grid of an imaginary-time kernel and its beta, which defaults to ``tau[-1]``"""
    tau = np.asarray(kernel.tau, dtype=float)
    return tau, (tau[-1] if kernel.beta is None else kernel.beta)


class TauKernel(Kernel):
    r"""Fermionic imaginary-time kernel
    :math:`K(\tau,\omega) = -e^{-\tau\omega}/(1+e^{-\beta\omega})`
    (reference kernels.py:210-280).  ``beta`` defaults to ``tau[-1]``."""

    kind = 'tau'
    has_device_entry = True
    scannable = True

    def __init__(self, tau, omega, beta=None, svd_backend='host'):
        super(TauKernel, self).__init__()
        self.tau = tau
        self.omega = omega
        self.beta = beta
        self.svd_backend = svd_backend
        self._fill_values()

    def _device_entry(self, preblur_b=0.0):
        tau, beta = _tau_and_beta(self)
        return 'mxe_kernel_svd', tau, (float(beta),), len(tau)

    def _inputs(self, w):
        return _tau_and_beta(self)

    def _compute(self, w, tau, beta):
        ww = w[np.newaxis, :] * np.ones((len(tau), 1))
        tt = tau[:, np.newaxis] * np.ones((1, len(w)))
        pos = ww >= 0.0
        K = np.empty(ww.shape)
        # two algebraically equal forms, each overflow-free on its half-axis
        K[pos] = -np.exp(-ww[pos] * tt[pos]) / (np.exp(-beta * ww[pos]) + 1.0)
        neg = np.logical_not(pos)
        K[neg] = -np.exp(ww[neg] * (beta - tt[neg])) / \
            (1.0 + np.exp(beta * ww[neg]))
        return K

    @property
    def data_variable(self):
        return self.tau

    @data_variable.setter
    def data_variable(self, value):
        self.tau = value


def stack_complex(z):
    """complex values (last axis n) as the stacked real ``[Re ; Im]`` (last axis 2 n): the data of a kernel whose rows
    are ``[Re K ; Im K]``"""
    z = np.asarray(z)
    return np.concatenate([z.real, z.imag], axis=-1).astype(float, copy=False)


class _StackedRows(object):
    """What the Matsubara kernels share: the complex ``n x n_omega`` kernel is held as the stacked real matrix
    ``[Re K ; Im K]`` of ``2 n`` rows (``stacked``), the data the same way; ``beta`` is remembered (default: from the
    spacing of the grid) and does not enter the matrix.  A kind that is real for some arguments sets ``stacked`` False
    there: ``n`` rows, ``fold`` and ``unfold`` the identity on real data."""

    stacked = True
    beta_in_matrix = False

    @property
    def n_iw(self):
        return len(self.data_variable)

    def get_beta(self):
        if self._beta is None:
            iw = np.asarray(self.data_variable, dtype=float)
            return 2 * np.pi / (iw[1] - iw[0])
        return self._beta

    def set_beta(self, beta):
        self._beta = beta

    beta = property(get_beta, set_beta)

    @property
    def K_complex(self):
        """the complex ``K`` (n x n_omega; the reference's ``K`` of an IOmegaKernel), unrotated; real-valued (but
        complex dtype) where the kernel is not stacked"""
        n = self.n_iw
        if not self.stacked:
            return self._K_unrotated + 0j
        return self._K_unrotated[:n] + 1j * self._K_unrotated[n:]

    def fold(self, x):
        """``x[..., :n] + 1j x[..., n:]`` (n = n_iw): stacked real data-space values as the complex data; the identity
        where the kernel is not stacked"""
        if not self.stacked:
            return x
        x = np.asarray(x)
        n = self.n_iw
        if x.shape[-1] != 2 * n:
            raise ValueError('fold: the last axis has %d values, not 2 x %d' % (x.shape[-1], n))
        return x[..., :n] + 1j * x[..., n:]

    def unfold(self, z):
        """complex data (last axis n_iw) as the stacked real vector ``[Re ; Im]`` (:func:`stack_complex`); the real part
        where the kernel is not stacked, whose data are real"""
        if not self.stacked:
            return z if not np.iscomplexobj(z) else np.asarray(z).real.astype(float, copy=False)
        return stack_complex(z)


class IOmegaKernel(_StackedRows, Kernel):
    r"""Fermionic Matsubara kernel :math:`K(i\omega_n, \omega) = 1/(i\omega_n - \omega)` (reference
    kernels.py:283-346), for a REAL spectral function: the complex rows become the stacked real matrix

    .. math::

        K = \begin{pmatrix} \mathrm{Re}\,K \\ \mathrm{Im}\,K \end{pmatrix}, \quad
        \mathrm{Re}\,K = \frac{-\omega}{\omega_n^2 + \omega^2}, \quad
        \mathrm{Im}\,K = \frac{-\omega_n}{\omega_n^2 + \omega^2}

    of ``2 n_iw`` rows, with the data stacked the same way, ``[Re G ; Im G]``: chi2 over the complex
    data is the ordinary chi2 of that real system, so the solver runs unchanged.  ``K``, ``K_delta``,
    ``U``, ``S``, ``V`` belong to the stacked matrix (the reference's ``K`` is complex: it is
    ``K_complex`` here).  ``iomega``: the real frequencies :math:`\omega_n`; ``beta`` defaults to
    :math:`2\pi/(\omega_1 - \omega_0)` and does not enter K."""

    kind = 'iomega'
    has_device_entry = True

    def __init__(self, iomega, omega, beta=None, svd_backend='host'):
        super(IOmegaKernel, self).__init__()
        self.iomega = iomega
        self.omega = omega
        self.beta = beta
        self.svd_backend = svd_backend
        self._fill_values()

    def _device_entry(self, preblur_b=0.0):
        iw = np.asarray(self.iomega, dtype=float)
        return 'mxe_kernel_svd_iw', iw, (), 2 * len(iw)

    def _inputs(self, w):
        return (np.asarray(self.iomega, dtype=float),)

    def _compute(self, w, iw):
        d = iw[:, np.newaxis] ** 2 + w[np.newaxis, :] ** 2           # (one w_n^2 + w^2 for both parts, as the device fill)
        return np.concatenate([-w[np.newaxis, :] / d, -iw[:, np.newaxis] / d])

    @property
    def data_variable(self):
        return self.iomega

    @data_variable.setter
    def data_variable(self, value):
        self.iomega = value


def _exp_of_product(a, b, extra=0.0):
    """``exp(a * b)`` with the rounding of the product given back: p = fl(a b), e = a b - p exactly (Dekker's product
    of Veltkamp halves), exp(p + e + extra) = exp(p) (1 + e + extra) to first order.  A plain ``exp(a * b)`` is off by
    |a b| 2^-53 relative -- 4e-14 at tau omega = 400; this is a few ulp whatever the argument."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    x = np.exp(p)
    return x + x * (e + extra)


def _require_half_axis(omega, name):
    if np.any(np.asarray(omega, dtype=float) < 0.0):
        raise ValueError('%s(symmetric=True) needs a mesh on omega >= 0: A(omega) = A(-omega) is continued on the '
                         'half-axis' % name)


#: below |beta omega| = this the factor beta omega / (1 - e^{-beta omega}) of the bosonic tau kernel is its series
#: 1 + x/2 + x^2/12 (next term x^4/720 < 2e-23); it covers omega = 0 exactly and products that underflow
BOSON_SERIES_CUT = 1.0e-5


class BosonicTauKernel(Kernel):
    r"""Bosonic imaginary-time kernel for :math:`A(\omega) = \mathrm{Im}\,\chi(\omega)/(\pi\omega)`:
    :math:`\chi(\tau) = \int d\omega\, K(\tau,\omega) A(\omega)`,

    .. math:: K(\tau,\omega) = \frac{\omega e^{-\tau\omega}}{1 - e^{-\beta\omega}}, \quad K(\tau, 0) = 1/\beta

    (positive: no sign as in the fermionic :class:`TauKernel`).  ``symmetric=True``: :math:`A(\omega) = A(-\omega)`
    on a mesh :math:`\omega \ge 0`, :math:`K_s(\tau,\omega) = K(\tau,\omega) + K(\tau,-\omega)`, 2/beta at 0.
    ``beta`` defaults to ``tau[-1]``.  Not in the reference (its FAQ anticipates it).

    The fill has no overflow on either half-axis (:math:`e^{-(\beta-\tau)|\omega|}` for negative omega), uses
    ``expm1`` for the denominator and a short series below ``BOSON_SERIES_CUT``, and compensates the rounding of the
    arguments of ``exp``: every entry is good to a few ulp."""

    kind = 'boson_tau'
    kind_params = ('symmetric',)
    has_device_entry = True
    scannable = True

    def __init__(self, tau, omega, beta=None, symmetric=False, svd_backend='host'):
        super(BosonicTauKernel, self).__init__()
        self.tau = tau
        self.omega = omega
        self.beta = beta
        self.symmetric = bool(symmetric)
        self.svd_backend = svd_backend
        self._fill_values()

    def _device_entry(self, preblur_b=0.0):
        tau, beta = _tau_and_beta(self)
        return 'mxe_kernel_svd_boson', tau, (float(beta), 1 if self.symmetric else 0), len(tau)

    @staticmethod
    def _values(tau, w, beta, symmetric):
        t = tau[:, np.newaxis] * np.ones((1, len(w)))
        ww = w[np.newaxis, :] * np.ones((len(tau), 1))
        x = beta * ww
        # beta - tau = bt + bt_lo exactly (two-sum)
        bt = beta - t
        bb = bt - beta
        bt_lo = (beta - (bt - bb)) + (-t - bb)
        K = np.empty(ww.shape)
        small = np.abs(x) < BOSON_SERIES_CUT
        s = small
        sp = 1.0 + 0.5 * x[s] + x[s] * x[s] / 12.0
        if symmetric:
            sn = 1.0 - 0.5 * x[s] + x[s] * x[s] / 12.0
            K[s] = sp * _exp_of_product(-t[s], ww[s]) / beta + sn * _exp_of_product(t[s], ww[s]) / beta
            r = np.logical_not(small)
            K[r] = ww[r] * (_exp_of_product(-t[r], ww[r]) + _exp_of_product(-bt[r], ww[r], -bt_lo[r] * ww[r])) / \
                (-np.expm1(-x[r]))
            return K
        K[s] = sp * _exp_of_product(-t[s], ww[s]) / beta
        # two algebraically equal forms, each overflow-free on its half-axis
        pos = np.logical_and(np.logical_not(small), ww > 0.0)
        K[pos] = ww[pos] * _exp_of_product(-t[pos], ww[pos]) / (-np.expm1(-x[pos]))
        neg = np.logical_and(np.logical_not(small), ww < 0.0)
        K[neg] = ww[neg] * _exp_of_product(bt[neg], ww[neg], bt_lo[neg] * ww[neg]) / np.expm1(x[neg])
        return K

    def _inputs(self, w):
        if self.symmetric:
            _require_half_axis(w, 'BosonicTauKernel')
        tau, beta = _tau_and_beta(self)
        return tau, float(beta), self.symmetric

    def _compute(self, w, tau, beta, symmetric):
        with np.errstate(under='ignore'):
            return self._values(tau, w, beta, symmetric)

    @property
    def data_variable(self):
        return self.tau

    @data_variable.setter
    def data_variable(self, value):
        self.tau = value


class BosonicIOmegaKernel(_StackedRows, Kernel):
    r"""Bosonic Matsubara kernel :math:`K(i\nu_n, \omega) = \omega/(\omega - i\nu_n)
    = (\omega^2 + i\omega\nu_n)/(\omega^2 + \nu_n^2)`, 1 at :math:`\omega = \nu_n = 0`, for
    :math:`A(\omega) = \mathrm{Im}\,\chi(\omega)/(\pi\omega)`; held like :class:`IOmegaKernel` as the stacked real
    matrix ``[Re K ; Im K]`` of ``2 n`` rows with ``K_complex``, ``fold``, ``unfold`` (the zero row
    Im K(i nu_0 = 0) is kept: the layout stays 2 n).  ``symmetric=True``: :math:`A(\omega) = A(-\omega)` on a mesh
    :math:`\omega \ge 0`, the real kernel :math:`2\omega^2/(\omega^2 + \nu_n^2)` of ``n`` rows (2 at the origin) for
    the data Re chi(i nu_n); ``fold`` / ``unfold`` are then the identity.  ``inu``: the real frequencies
    :math:`\nu_n = 2\pi n/\beta`; ``beta`` defaults to :math:`2\pi/(\nu_1 - \nu_0)` and does not enter K."""

    kind = 'boson_iomega'
    kind_params = ('symmetric',)
    has_device_entry = True

    def __init__(self, inu, omega, beta=None, symmetric=False, svd_backend='host'):
        super(BosonicIOmegaKernel, self).__init__()
        self.inu = inu
        self.omega = omega
        self.beta = beta
        self.symmetric = bool(symmetric)
        self.svd_backend = svd_backend
        self._fill_values()

    @property
    def stacked(self):
        """whether the rows are ``[Re K ; Im K]`` (2 n of them) and the data complex"""
        return not self.symmetric

    def _device_entry(self, preblur_b=0.0):
        nu = np.asarray(self.inu, dtype=float)
        return 'mxe_kernel_svd_boson_iw', nu, (1 if self.symmetric else 0,), len(nu) if self.symmetric else 2 * len(nu)

    def _inputs(self, w):
        if self.symmetric:
            _require_half_axis(w, 'BosonicIOmegaKernel')
        return np.asarray(self.inu, dtype=float), self.symmetric

    def _compute(self, w, nu, symmetric):
        w2 = (w * w)[np.newaxis, :]
        d = nu[:, np.newaxis] ** 2 + w2                  # (one nu_n^2 + w^2 for both parts, as the device fill)
        origin = np.logical_not(d > 0.0)                 # (w = nu_n = 0: K = 1)
        with np.errstate(invalid='ignore', divide='ignore', under='ignore'):
            if symmetric:
                return np.where(origin, 2.0, 2.0 * w2 / d)
            return np.concatenate([np.where(origin, 1.0, w2 / d),
                                   np.where(origin, 0.0, w[np.newaxis, :] * nu[:, np.newaxis] / d)])

    @property
    def data_variable(self):
        return self.inu

    @data_variable.setter
    def data_variable(self, value):
        self.inu = value


#: below a = beta |omega| / 2 = this the scaled e^{-a} i_0(a) = (1 - e^{-2a}) / (2a) of the Legendre kernel is its series
#: 1 - a + 2 a^2 / 3 (next term a^3 / 3 < 4e-19); it covers omega = 0 exactly (no 0 / 0) and products that underflow
LEGENDRE_SERIES_CUT = 1.0e-6
#: the backward recurrence of the ratios starts at L = m + LEGENDRE_START_PAD + floor(LEGENDRE_START_SQRT sqrt(m)),
#: m = max(l_max, floor(a)); see :func:`_legendre_start`
LEGENDRE_START_PAD = 40
LEGENDRE_START_SQRT = 6.0
#: largest order l a LegendreKernel (and ``mxe_kernel_svd_legendre``) takes
LEGENDRE_L_MAX = 4096
#: largest a = beta |omega| / 2 they take: the work of a column grows like max(l_max, a)
LEGENDRE_A_MAX = 1.0e6


def _legendre_start(l_max, a):
    """The order L at which the backward recurrence of the ratios r_k = i_{k+1}(a) / i_k(a) starts with r_L = 0.

    An error e_k of r_k becomes e_{k-1} = -r_{k-1}^2 e_k one step down (differentiate r_{k-1} = a / (2k + 1 + a r_k)), so
    the wrong start (relative error 1) arrives at order l multiplied by prod_{k=l+1..L} r_{k-1} r_k.  Above the turning
    point k ~ a the ratios fall like r_k < a / (2k + 3): with m = max(l, a) and k = m + d, r_k < 1 / (1 + 2d / m)
    ~ exp(-2d / m) for d << m, the product over d = 1..D is below exp(-2 D^2 / m), and D = 6 sqrt(m) alone gives
    e^-72 ~ 5e-32; for d >~ m every factor is below 1/2 and 40 further steps give 2^-80 for small m, where sqrt(m) is
    no measure.  Either term suffices on its side; their sum is used for all m, far below 2^-53 everywhere."""
    m = np.maximum(float(l_max), np.floor(a))
    return (m + LEGENDRE_START_PAD + np.floor(LEGENDRE_START_SQRT * np.sqrt(m))).astype(np.int64)


class LegendreKernel(Kernel):
    r"""Fermionic kernel for G given as Legendre coefficients :math:`G_l` in TRIQS's ``GfLegendre`` normalisation,
    :math:`G(\tau) = \sum_l \sqrt{2l+1}/\beta\; P_l(x(\tau))\, G_l`, :math:`x(\tau) = 2\tau/\beta - 1`:
    :math:`G_l = \int d\omega\, K(l,\omega) A(\omega)` with

    .. math:: K(l,\omega) = -\beta\sqrt{2l+1}\,(-\mathrm{sgn}\,\omega)^l\,
              \frac{i_l(\beta|\omega|/2)}{2\cosh(\beta\omega/2)}

    (:math:`i_l`: the modified spherical Bessel function of the first kind); :math:`K(0,\omega) =
    -\tanh(\beta\omega/2)/\omega`, and at :math:`\omega = 0` the row l = 0 is :math:`-\beta/2`, every other row 0.
    ``l``: distinct non-negative integers in any order (a subset such as the even l is fine); ``beta`` is required.
    The matrix is real with ``len(l)`` rows.  Not in the reference (its documentation anticipates it).

    The fill runs column by column in :math:`a = \beta|\omega|/2`: the ratios :math:`r_{k-1} = i_k/i_{k-1} =
    a/(2k+1+a r_k)` backwards from :math:`r_L = 0` (:func:`_legendre_start`), the scaled :math:`s_0 = e^{-a} i_0(a) =
    -\mathrm{expm1}(-2a)/(2a)` (a series below ``LEGENDRE_SERIES_CUT``), :math:`s_{k+1} = s_k r_k` forwards, and
    :math:`K = -\beta\sqrt{2l+1}(-\mathrm{sgn}\,\omega)^l s_l/(1+e^{-2a})`.  No exponent is positive: nothing
    overflows for any :math:`\beta\omega`, small entries underflow to 0.  The work per column grows like
    :math:`\max(l_{max}, a)`."""

    kind = 'legendre'
    has_device_entry = True
    scannable = True

    def __init__(self, l, omega, beta=None, svd_backend='host'):
        super(LegendreKernel, self).__init__()
        self._checked_beta(beta)
        self.l = self._checked_l(l)
        self.omega = omega
        self.beta = beta
        self.svd_backend = svd_backend
        self._fill_values()

    @staticmethod
    def _checked_beta(beta):
        """raises ValueError naming ``beta`` unless it is a positive finite number"""
        if beta is None:
            raise ValueError('LegendreKernel: beta is required (it is not in the grid l)')
        if not (float(beta) > 0.0 and np.isfinite(float(beta))):
            raise ValueError('LegendreKernel: beta must be positive and finite, not %r' % (beta,))
        return beta

    @staticmethod
    def _checked_l(l):
        """``l`` as an int64 array; raises ValueError naming ``l`` for anything but distinct non-negative integers"""
        a = np.asarray(l)
        if a.ndim != 1 or a.size < 1:
            raise ValueError('LegendreKernel: l must be a 1-D array of orders, not of shape %s' % (a.shape,))
        if a.dtype.kind not in 'iuf' or not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
            raise ValueError('LegendreKernel: l must hold integers')
        if np.any(a < 0):
            raise ValueError('LegendreKernel: l must not be negative')
        if np.any(a > LEGENDRE_L_MAX):
            raise ValueError('LegendreKernel: l must not exceed %d' % LEGENDRE_L_MAX)
        a = a.astype(np.int64)
        if len(np.unique(a)) != len(a):
            raise ValueError('LegendreKernel: l holds duplicates')
        return a

    @classmethod
    def _checked_args(cls, grid, beta=None):
        cls._checked_beta(beta)
        return cls._checked_l(grid)

    def _device_entry(self, preblur_b=0.0):
        return 'mxe_kernel_svd_legendre', self.l, (float(self.beta),), len(self.l)

    @staticmethod
    def _scaled_bessel(l_max, a):
        """s_k = e^{-a} i_k(a) for k = 0..l_max and every a >= 0 of the array ``a``: (l_max + 1, len(a))"""
        L = _legendre_start(l_max, a)
        r = np.zeros(len(a))
        ratios = np.empty((l_max + 1, len(a)))
        for k in range(int(L.max()), 0, -1):
            # r holds r_k (0 where k >= L: the recurrence of that column has not started)
            r = np.where(k <= L, a / ((2 * k + 1) + a * r), 0.0)
            if k - 1 <= l_max:
                ratios[k - 1] = r
        small = a < LEGENDRE_SERIES_CUT
        s = np.empty((l_max + 1, len(a)))
        s[0] = np.where(small, 1.0 - a + 2.0 * a * a / 3.0, -np.expm1(-2.0 * a) / np.where(small, 1.0, 2.0 * a))
        for k in range(l_max):
            s[k + 1] = s[k] * ratios[k]
        return s

    @classmethod
    def _values(cls, l, w, beta):
        a = beta * np.abs(w) / 2.0
        s = cls._scaled_bessel(int(l.max()), a)[l]
        c = -beta * np.sqrt(2.0 * l + 1.0)
        # (-sgn omega)^l: -1 for odd l on omega > 0, +1 otherwise
        sign = np.where((l[:, np.newaxis] % 2 == 1) & (w[np.newaxis, :] > 0.0), -1.0, 1.0)
        return sign * (c[:, np.newaxis] * s / (1.0 + np.exp(-2.0 * a))[np.newaxis, :])

    def _inputs(self, w):
        l = self._checked_l(self.l)
        beta = float(self.beta)
        if not np.all(beta * np.abs(w) / 2.0 <= LEGENDRE_A_MAX):                # (also a NaN)
            raise ValueError('LegendreKernel: beta |omega| / 2 must not exceed %g' % LEGENDRE_A_MAX)
        return l, beta

    def _compute(self, w, l, beta):
        with np.errstate(under='ignore'):
            return self._values(l, w, beta)

    @property
    def data_variable(self):
        return self.l

    @data_variable.setter
    def data_variable(self, value):
        self.l = self._checked_l(value)


class PreblurKernel(Kernel):
    """``K' = K diag(delta) B`` for the preblur formalism; ``K_delta`` stays
    un-blurred (reference kernels.py:349-413)."""

    def __init__(self, K, b, svd_backend=None):
        KernelSVD.__init__(self)
        self._T = None
        self.kernel = K
        self._b = b
        self.svd_backend = K.svd_backend if svd_backend is None else svd_backend
        self._fill_values()

    def fold(self, x):
        return self.kernel.fold(x)

    def unfold(self, x):
        return self.kernel.unfold(x)

    def _device_svd(self):
        if not getattr(self.kernel, 'has_device_entry', False):
            raise NotImplementedError('device SVD of a PreblurKernel needs a kernel of this module inside')
        U, S, V = self.kernel._device_svd(preblur_b=self._b)
        T = self.kernel._T
        return (U if T is None else np.dot(T, U)), S, V

    @classmethod
    def scan(cls, K, b_values, threshold=1.e-14):
        """The kernels of a b-scan (reference doc/guide/preblur_example.py:49-56) with
        their truncated SVDs from ONE batched device launch (``mxe_kernel_svd``, ``mxe_kernel_svd_boson``
        for a BosonicTauKernel, ``mxe_kernel_svd_legendre`` for a LegendreKernel)."""
        from . import device
        if not getattr(K, 'scannable', False) or K._T is not None:
            raise NotImplementedError('PreblurKernel.scan needs an unrotated TauKernel, BosonicTauKernel or LegendreKernel')
        name, grid, scalars, n_rows = K._device_entry()
        res = device._kernel_svd(name, grid, scalars, np.asarray(K.omega, dtype=float), K.omega.delta,
                                 list(b_values), threshold=threshold, n_rows=n_rows)
        out = []
        for b, r in zip(b_values, res):
            Kb = cls(K, b, svd_backend='device')
            Kb._U, Kb._S, Kb._V = r['U'], r['S'], r['V']
            Kb._last_threshold = threshold
            out.append(Kb)
        return out

    def parameter_change(self):
        self.kernel.parameter_change()
        self._fill_values()

    def refill_unrotated(self):
        self.kernel.refill_unrotated()
        self._fill_values()

    def _fill_values(self):
        self._invalidate_svd()
        self._B = get_preblur(self.omega, self._b)
        self._K = np.dot(self.kernel.K,
                         self._B * self.omega.delta[:, np.newaxis])
        self._K_delta = self.kernel.K_delta

    def transform(self, T):
        """rotate the blurred kernel like the plain one: ``U <- T U``, ``K <- T K``, S and V stay.  (The
        reference refills and decomposes T K' again for every rotation, kernels.py:395-397; the
        decomposition of the unrotated K' spans every rotated kernel's row space, so one V serves all
        matrix elements of a job and the SVD is done once.)"""
        rel = self._relative_rotation(T, self.kernel._T)
        if rel is None:
            return
        U = self.U
        self.kernel.transform(T)
        self._U = np.dot(rel, U)
        self._K = np.dot(rel, self._K)

    # ``_T`` of a PreblurKernel stays None in the reference (kernels.py:374: only the wrapped kernel's is
    # updated), and TauMaxEnt's bookkeeping of the DATA rotation reads it: with a preblur the data are
    # never rotated back before a new rotation.  The results of the reference depend on it
    # (tests/golden/elementwise_cov.npz), so it is kept; the rotation the matrix really carries is
    # ``rotation``.
    @property
    def rotation(self):
        return self.kernel.rotation

    @property
    def b(self):
        return self._b

    @b.setter
    def b(self, value):
        # (reference test/python/cov.py:158-159 assigns ``K.b`` and calls ``parameter_change()``; in the reference the
        #  assignment creates an attribute nobody reads and the refill blurs with the old width -- here it is the width)
        self._b = value

    @property
    def B(self):
        return self._B

    def get_omega(self):
        return self.kernel.omega

    def set_omega(self, omega):
        self.kernel.omega = omega

    omega = property(get_omega, set_omega)

    @property
    def data_variable(self):
        return self.kernel.data_variable

    @data_variable.setter
    def data_variable(self, value):
        self.kernel.data_variable = value
